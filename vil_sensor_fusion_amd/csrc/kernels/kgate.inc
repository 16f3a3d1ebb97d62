// kernels/kgate.inc -- k_gate_between: the innovation test of a between factor BEFORE it enters the graph -- how many sigmas an
// odometry increment lies from where the window as solved, and the IMU since, expect it (DESIGN.md section 4g).
// A section of vf_kernels.hip (ONE translation unit); included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ k_gate_between
// One 256-thread workgroup per window, the LDS plan of k_propagate plus a few small blocks.  For window w, its last keyframe
// i = hi[w] - 1, the raw samples steps[off[w] .. off[w + 1]) that follow it and a candidate BetweenFactor<Pose3> from slot a = btw_a[w]
// to the keyframe j those samples lead to (record: the 28 words vf_engine_ingest_tail takes):
//   (a), (b) k_propagate's own routines (kprop.inc): mean, H, P; the predicted state x_j -- the bits vf_engine_propagate_tail gives;
//   (c) the appended keyframe's linear model A d_i + B d_j = n, n ~ N(0, P), hence d_j = G d_i + B^-1 n, G = -B^-1 A.  B =
//       -diag(I, I, R_j^T, I, I) touches the velocity rows only, so the pose rows G_p are the first six rows of A (tests/gate_ref.py
//       checks that against -B^-1 A in extended precision).  With Sigma_{i,a} = Cov(x_i, x_a):
//           Sigma_jj^pp = (A Sigma_ii A^T + P)[0:6, 0:6]              C = Cov(pose_j, pose_a) = (G_p Sigma_{i,a})[:, 0:6]
//       a = i: Sigma_{i,a} = Sigma_ii; a = i - 1: the cross block of slot i - 1 of sig (row = dof of i).  n is independent of the
//       window, so no other block is needed.  An older a would need an earlier pose against a later full state, which the profile
//       of the selected inversion does not hold (k4_selinv.inc): out of reach, a status;
//   (d) K2's value-level routine (between_values, k12_linearize.inc) at T_a of the current buffer and the predicted T_j: the
//       whitened residual r, Ja, Jb, and the unwhitened innovation xi = Log(Z^-1 T_a^-1 T_j);
//   (e) S = I + [Ja Jb] [[Sigma_aa^pp, C^T], [C, Sigma_jj^pp]] [Ja Jb]^T, symmetrised; nis = r^T S^-1 r by a 6 x 6 Cholesky
//       factorisation, nis_measurement = r^T r.
// No samples: x_j is keyframe i, copied (a = i is then the factor of a keyframe with itself: degenerate); A = I and P = 0 go through
// the same products, exactly.  Only out[w] is written.
struct GateOut {
    unsigned struct_size;      // (the caller's word of vf_gate_result: never written on the device beyond a zero)
    int status, rejected, reserved;
    double nis, nis_measurement, xi[6], state[16];
};
constexpr int GATE_OK = 0, GATE_NONE = 1, GATE_OUT_OF_REACH = 2, GATE_DEGENERATE = 3, GATE_NO_COVARIANCE = 4;   // VF_GATE_*

// where thread 0 leaves (d): the 6 x 12 block [Ja Jb] and r in LDS
struct GateSink {
    double* J;
    double* r6;
    VF_DI void r(int f, double x) { r6[f] = x; }
    VF_DI void ja(int e, double x) { J[(e / 6) * 12 + e % 6] = x; }
    VF_DI void jb(int e, double x) { J[(e / 6) * 12 + 6 + e % 6] = x; }
};

// (e) of k_gate_between, shared with k_gate_closure (kclosure.inc): S = I + [Ja Jb] Sigma_J [Ja Jb]^T, symmetrised, from sJ (6 x 12) and
// sJoint (12 x 12) in LDS; then on thread 0 S = L L^T, y = L^-1 r, nis = y^T y and m = r^T r.  The whole workgroup calls it (72 threads
// at least; it synchronises, and sJ, sR, sJoint are complete when it is entered); nis, m and the value returned are thread 0's.
// false: a pivot was not positive.
VF_DI bool gate_nis(int tid, const double* sJ, const double* sR, const double* sJoint, double* sU, double* sSm, double& nis, double& m) {
    if (tid < 72) {
        const int r = tid / 12, c = tid - r * 12;
        double x = 0.0;
        for (int l = 0; l < 12; l++) x = fma(sJ[r * 12 + l], sJoint[l * 12 + c], x);
        sU[tid] = x;
    }
    __syncthreads();
    if (tid < 36) {
        const int r = tid / 6, c = tid - r * 6;
        double x = 0.0, y = 0.0;
        for (int l = 0; l < 12; l++) {
            x = fma(sU[r * 12 + l], sJ[c * 12 + l], x);
            y = fma(sU[c * 12 + l], sJ[r * 12 + l], y);
        }
        sSm[tid] = (r == c ? 1.0 : 0.0) + 0.5 * (x + y);
    }
    __syncthreads();
    bool spd = true;
    nis = 0.0, m = 0.0;
    if (tid == 0) {
        double S[36], L[36], r6[6], y[6];
#pragma unroll
        for (int e = 0; e < 36; e++) S[e] = sSm[e];
#pragma unroll
        for (int e = 0; e < 6; e++) r6[e] = sR[e];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double d = S[c * 6 + c];
#pragma unroll
            for (int k = 0; k < c; k++) d = fma(-L[c * 6 + k], L[c * 6 + k], d);
            if (!(d > 0.0)) spd = false;
            const double lcc = sqrt(d), inv = 1.0 / lcc;
#pragma unroll
            for (int r = c + 1; r < 6; r++) {
                double x = S[r * 6 + c];
#pragma unroll
                for (int k = 0; k < c; k++) x = fma(-L[r * 6 + k], L[c * 6 + k], x);
                L[r * 6 + c] = x * inv;
            }
            double x = r6[c];
#pragma unroll
            for (int k = 0; k < c; k++) x = fma(-L[c * 6 + k], y[k], x);
            y[c] = x * inv;
            nis = fma(y[c], y[c], nis);
            m = fma(r6[c], r6[c], m);
        }
    }
    return spd;
}

__global__ void __launch_bounds__(256) k_gate_between(View v, const int* __restrict__ off, const double* __restrict__ steps, ImuCov prm,
                                                     const int* __restrict__ btw_a, const int* __restrict__ reach_lo,
                                                     const double* __restrict__ btw_rec, double threshold, int from_estimate,
                                                     const double* __restrict__ sig, const int* __restrict__ sig_failed,
                                                     GateOut* __restrict__ out) {
    const int w = blockIdx.x, tid = threadIdx.x;
    if (w >= v.B) return;
    __shared__ double sF[225], sP[225], sT[225], sS[225], sA[225], sH[54], sHn[54];
    __shared__ double sJ[72], sR[6], sJoint[144], sU[72], sSm[36], sT2[90];
    const int i = tid / 15, j = tid - i * 15;          // entry of the 15x15 matrices (tid < 225)
    GateOut* o = out + w;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int hi_w = v.hi[w], lo_w = v.lo[w];
    if (hi_w <= lo_w || hi_w > v.M) {                  // empty window: nothing to start from (the engine refuses such a call)
        if (tid < 16) o->state[tid] = qnan;
        if (tid < 6) o->xi[tid] = qnan;
        if (tid == 0) { o->struct_size = 0; o->status = GATE_NONE; o->rejected = 0; o->reserved = 0; o->nis = qnan; o->nis_measurement = qnan; }
        return;
    }
    const int ik = hi_w - 1;
    const long gk = (long)w * v.M + ik;
    const int b = v.sel[w], bs = from_estimate ? b ^ 1 : b;
    const int s0 = off[w], s1 = off[w + 1];
    const bool samples = s1 > s0;
    const int a = btw_a[w];
    // (a), (b)
    State sj;
    ImuPrediction p{};
    if (samples) {
        double bh[6];
#pragma unroll
        for (int c = 0; c < 6; c++) bh[c] = XS(b, 10 + c, gk);
        const V3 bacc = v3(bh[0], bh[1], bh[2]), bgyr = v3(bh[3], bh[4], bh[5]);
        const PropMean pm = prop_integrate(steps, s0, s1, bacc, bgyr, prm, sF, sP, sT, sH, sHn);
        const State si = load_state(v, bs, gk);
        p = prop_predict(v, si, pm, bh, sH);
        sj = predicted_state(si, p);
    } else {
        sj = load_state(v, bs, gk);
    }
    if (tid == 0) {
        o->state[0] = sj.q.w; o->state[1] = sj.q.x; o->state[2] = sj.q.y; o->state[3] = sj.q.z;
        o->state[4] = sj.t.x; o->state[5] = sj.t.y; o->state[6] = sj.t.z;
        o->state[7] = sj.vel.x; o->state[8] = sj.vel.y; o->state[9] = sj.vel.z;
        o->state[10] = sj.ba.x; o->state[11] = sj.ba.y; o->state[12] = sj.ba.z;
        o->state[13] = sj.bg.x; o->state[14] = sj.bg.y; o->state[15] = sj.bg.z;
    }
    // what the window can answer (uniform over the workgroup)
    int status = GATE_OK;
    if (a == -1) status = GATE_NONE;
    else if (a > ik || a < ik - 1 || a < lo_w || a < reach_lo[w]) status = GATE_OUT_OF_REACH;
    else if (a == ik && !samples) status = GATE_DEGENERATE;
    if (status != GATE_OK) {
        if (tid < 6) o->xi[tid] = qnan;
        if (tid == 0) { o->struct_size = 0; o->status = status; o->rejected = 0; o->reserved = 0; o->nis = qnan; o->nis_measurement = qnan; }
        return;
    }
    const bool cov_bad = sig_failed[w] != 0;
    const long ga = (long)w * v.M + a;
    // (d) on thread 0, beside (c) on the others
    Xi6 xi{};
    if (tid == 0) {
        const Q4 qa = q4(XS(b, 0, ga), XS(b, 1, ga), XS(b, 2, ga), XS(b, 3, ga));
        const V3 ta = v3(XS(b, 4, ga), XS(b, 5, ga), XS(b, 6, ga));
        const double* __restrict__ rec = btw_rec + (size_t)w * BTW_IN;
        GateSink sink{sJ, sR};
        xi = between_values(qa, ta, sj.q, sj.t, [rec](int f) { return rec[f]; }, sink);
    }
    if (cov_bad) {                                     // the window's factorisation failed: the innovation without its covariance
        if (tid == 0) {
            double m = 0.0;
            for (int r = 0; r < 6; r++) m = fma(sR[r], sR[r], m);
            o->xi[0] = xi.w.x; o->xi[1] = xi.w.y; o->xi[2] = xi.w.z; o->xi[3] = xi.u.x; o->xi[4] = xi.u.y; o->xi[5] = xi.u.z;
            o->struct_size = 0; o->status = GATE_NO_COVARIANCE; o->rejected = 0; o->reserved = 0; o->nis = qnan; o->nis_measurement = m;
        }
        return;
    }
    // (c) the pose rows of A, Sigma_ii into sF, Sigma_{i,a} into sS
    const double* __restrict__ sgi = sig + (size_t)gk * SIG_SLOT;
    const double* __restrict__ sga = sig + (size_t)ga * SIG_SLOT;
    if (samples) __syncthreads();                      // (sF, sT were prop_integrate's scratch)
    if (tid < 225) {
        if (!samples) sP[tid] = 0.0;
        if (i < 6) sA[tid] = samples ? prop_A_entry(sj, p, sH, i, j) : (i == j ? 1.0 : 0.0);
        const double x = sgi[i >= j ? h_tri(i, j) : h_tri(j, i)];
        sF[tid] = x;
        sS[tid] = a == ik ? x : sga[120 + tid];
    }
    __syncthreads();
    if (tid < 90) {
        double c = 0.0, t = 0.0;
        for (int l = 0; l < 15; l++) {
            c = fma(sA[i * 15 + l], sS[l * 15 + j], c);
            t = fma(sA[i * 15 + l], sF[l * 15 + j], t);
        }
        sT[tid] = c;       // G_p Sigma_{i,a}
        sT2[tid] = t;      // G_p Sigma_ii
    }
    __syncthreads();
    if (tid < 36) {        // the joint pose covariance of (a, j), 12 x 12: [[Sigma_aa^pp, C^T], [C, Sigma_jj^pp]]
        const int pr = tid / 6, pc = tid - pr * 6;
        double x = 0.0, y = 0.0;
        for (int l = 0; l < 15; l++) {
            x = fma(sT2[pr * 15 + l], sA[pc * 15 + l], x);
            y = fma(sT2[pc * 15 + l], sA[pr * 15 + l], y);
        }
        x += sP[pr * 15 + pc];
        y += sP[pc * 15 + pr];
        sJoint[(6 + pr) * 12 + 6 + pc] = 0.5 * (x + y);
        sJoint[pr * 12 + pc] = sga[pr >= pc ? h_tri(pr, pc) : h_tri(pc, pr)];
        const double c = sT[pr * 15 + pc];
        sJoint[(6 + pr) * 12 + pc] = c;
        sJoint[pc * 12 + 6 + pr] = c;
    }
    __syncthreads();
    // (e)
    double nis, m;
    const bool spd = gate_nis(tid, sJ, sR, sJoint, sU, sSm, nis, m);
    if (tid == 0) {
        if (!spd) nis = qnan;
        o->xi[0] = xi.w.x; o->xi[1] = xi.w.y; o->xi[2] = xi.w.z; o->xi[3] = xi.u.x; o->xi[4] = xi.u.y; o->xi[5] = xi.u.z;
        o->struct_size = 0;
        o->status = spd ? GATE_OK : GATE_NO_COVARIANCE;
        o->rejected = spd && nis > threshold ? 1 : 0;
        o->reserved = 0;
        o->nis = nis;
        o->nis_measurement = m;
    }
}
void launch_gate_between(const View& v, const int* off, const double* steps, const ImuCov& prm, const int* btw_a, const int* reach_lo,
                         const double* btw_rec, double threshold, int from_estimate, const double* sig, const int* sig_failed,
                         void* out, hipStream_t s) {
    hipLaunchKernelGGL(k_gate_between, dim3(v.B), dim3(256), 0, s, v, off, steps, prm, btw_a, reach_lo, btw_rec, threshold, from_estimate,
                       sig, sig_failed, (GateOut*)out);
}
