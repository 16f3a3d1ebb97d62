// kernels/kprop.inc -- k_propagate: the state between two solves, at IMU rate, with the covariance the graph would give it.
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ k_propagate
// One 256-thread workgroup per window, as K0 (whose note says why lane-per-factor 15 x 15 work was abandoned).  For window w and
// the raw samples steps[off[w] .. off[w + 1]) that follow its last keyframe i = hi[w] - 1:
//   (a) integrate them as K0's ingest form does -- the bias of keyframe i in the current buffer, the same step update in the same
//       accumulation order: mean, 9 x 6 bias Jacobians, 15 x 15 covariance P (no reverse Cholesky: P itself is wanted);
//   (b) predict the state by imu_predict, as k_predict does, the record's words taken from where they are (registers, sH), from
//       keyframe i of the current buffer or, from_estimate, of the trial buffer (reference-compat engines: the estimate, as
//       k_predict(from_trial));
//   (c) with_cov: Sigma+ = B^-1 (A Sigma_ii A^T + P) B^-T, A and B the unwhitened Jacobians of the combined-IMU factor's residual
//       with respect to keyframe i and the predicted keyframe j (the closed forms of linearize_imu_core at x_j = predicted: r_theta = 0,
//       L = I, R_j^T R_i = E^T), Sigma_ii the block the last vf_engine_marginals_ex left.  B = -diag(I, I, R_j^T, I, I): its inverse
//       rotates the velocity rows.  This is the marginal of a keyframe attached to the window by this factor alone, at zero residual.
// F, P, Sigma, A and the products live in LDS (5 x 225 + 2 x 54 doubles, 9.9 KB), thread (i, j) owns entry (i, j); no scratch (pick9).
// No samples: the keyframe's state and Sigma_ii are copied, bit for bit -- F = I, P = 0 pass through no arithmetic.
// out: [B][16 + 225].  A window whose marginals failed (sig_failed) gets a NaN covariance and a valid state; an empty window NaNs.
//
// Steps (a), (b) and the entries of A are routines of their own, one copy each: k_gate_between (kernels/kgate.inc) calls them too.
// (a): the samples steps[s0 .. s1), s1 > s0, integrated from zero with the biases (bacc, bgyr).  Every thread of the 256-thread workgroup calls it; on return P is in sP, the
// 9 x 6 bias Jacobians in sH (behind a barrier), the mean and the summed dt in every thread's registers.  sF, sT, sHn: scratch.
struct PropMean { V3 th, pos, vel; double dtij; };
__device__ __forceinline__ PropMean prop_integrate(const double* __restrict__ steps, const int s0, const int s1, const V3 bacc, const V3 bgyr,
                                                   const ImuCov& prm, double* sF, double* sP, double* sT, double* sH, double* sHn) {
    const int tid = threadIdx.x;
    const int i = tid / 15, j = tid - i * 15;          // entry of the 15x15 matrices (tid < 225)
    const int hi_ = tid / 6, hj = tid - hi_ * 6;       // entry of the 9x6 bias Jacobian (tid < 54)
    V3 th = v3(0, 0, 0), pos = v3(0, 0, 0), vel = v3(0, 0, 0);
    double dtij = 0.0;
    if (tid < 225) sP[tid] = 0.0;
    if (tid < 54) sH[tid] = 0.0;
    __syncthreads();
    for (int s = s0; s < s1; s++) {
        const double* st = steps + (size_t)s * 7;
        const double dt = st[0], dt22 = 0.5 * dt * dt;
        const V3 acc = v3(st[1], st[2], st[3]) - bacc, om = v3(st[4], st[5], st[6]) - bgyr;
        const M3 Jr = so3_jr(th), invD = so3_jr_inv(th);
        const V3 wt = mul(invD, om);
        const M3 R = qrot(qexp(th));
        const V3 anav = mul(R, acc);
        const M3 wH = mul(invD, so3_jr_apply_dtheta(th, wt));   // -w_tangent_H_theta
        const M3 aH = mul(mulSkew(R, neg(acc)), Jr);            // a_nav_H_theta
        // F = [[A, Fb], [0, I]]
        if (tid < 225) {
            double x = i == j ? 1.0 : 0.0;
            if (i < 3 && j < 3) x -= pick9(wH, i * 3 + j) * dt;
            if (i >= 3 && i < 6 && j < 3) x = pick9(aH, (i - 3) * 3 + j) * dt22;
            if (i >= 6 && i < 9 && j < 3) x = pick9(aH, (i - 6) * 3 + j) * dt;
            if (i < 3 && j >= 12) x = -pick9(invD, i * 3 + j - 12) * dt;
            if (i >= 6 && i < 9 && j >= 9 && j < 12) x = -pick9(R, (i - 6) * 3 + j - 9) * dt;
            if (i >= 3 && i < 6 && j == i + 3) x = dt;
            sF[tid] = x;
        }
        __syncthreads();
        // bias Jacobians: H <- A H - [B | C]
        if (tid < 54) {
            double a = 0.0;
            for (int l = 0; l < 9; l++) a = fma(sF[hi_ * 15 + l], sH[l * 6 + hj], a);
            if (hi_ >= 3 && hi_ < 6 && hj < 3) a -= pick9(R, (hi_ - 3) * 3 + hj) * dt22;
            if (hi_ >= 6 && hj < 3) a -= pick9(R, (hi_ - 6) * 3 + hj) * dt;
            if (hi_ < 3 && hj >= 3) a -= pick9(invD, hi_ * 3 + hj - 3) * dt;
            sHn[tid] = a;
        }
        // covariance: P <- F P F^T + G Q G^T
        if (tid < 225) {
            double a = 0.0;
            for (int l = 0; l < 15; l++) a = fma(sF[i * 15 + l], sP[l * 15 + j], a);
            sT[tid] = a;
        }
        __syncthreads();
        if (tid < 54) sH[tid] = sHn[tid];
        if (tid < 225) {
            double a = 0.0;
            for (int l = 0; l < 15; l++) a = fma(sT[i * 15 + l], sF[j * 15 + l], a);
            const double sv = (prm.acc + prm.bias_int) * dt, sr = (prm.gyro + prm.bias_int) * dt;
            if (i >= 6 && i < 9 && j >= 6 && j < 9) {
                const M3 RRt = mulBT(R, R);
                a += sv * pick9(RRt, (i - 6) * 3 + j - 6);
            }
            if (i < 3 && j < 3) {
                const M3 DDt = mulBT(invD, invD);
                a += sr * pick9(DDt, i * 3 + j);
            }
            if (i == j && i >= 3 && i < 6) a += dt * prm.integration;
            if (i == j && i >= 9 && i < 12) a += dt * prm.bias_acc;
            if (i == j && i >= 12) a += dt * prm.bias_omega;
            sP[tid] = a;
        }
        // mean
        th = th + dt * wt;
        pos = pos + dt * vel + dt22 * anav;
        vel = vel + dt * anav;
        dtij += dt;
        __syncthreads();
    }
    return PropMean{th, pos, vel, dtij};
}
// (b) the prediction from keyframe i's state si: the record's words taken from where prop_integrate left them
__device__ __forceinline__ ImuPrediction prop_predict(const View& v, const State& si, const PropMean& pm, const double (&bh)[6], const double* sH) {
    const V3 th = pm.th, pos = pm.pos, vel = pm.vel;
    const double dtij = pm.dtij;
    const double mean[9] = {th.x, th.y, th.z, pos.x, pos.y, pos.z, vel.x, vel.y, vel.z};
    return imu_predict(v, si, [&](int f) { return f == 0 ? dtij : (f < 10 ? mean[f - 1] : (f < 16 ? bh[f - 10] : sH[f - 16])); });
}
// (c) entry (i, j) of A, the unwhitened Jacobian of the combined-IMU factor's residual with respect to keyframe i at x_j = predicted
// (sj, p: the predicted state and the prediction it was made from; sH: the bias Jacobians prop_integrate left)
__device__ __forceinline__ double prop_A_entry(const State& sj, const ImuPrediction& p, const double* sH, const int i, const int j) {
    const M3 Rj = qrot(sj.q);
    const M3 Rji = mulTA(Rj, p.Ri);             // R_j^T R_i
    const int bi = i / 3, r = i - bi * 3, bj = j / 3, c = j - bj * 3;
    double x = 0.0;
    if (i >= 9) x = i == j ? 1.0 : 0.0;        // bias rows: b_i - b_j
    else if (j < 9) {
        if (bj == 0) {
            const M3 X = bi == 0 ? transpose(qrot(qexp(p.tht))) : mulSkew(Rji, neg(bi == 1 ? p.pt : p.vt));   // E^T, -R_ji [p~]x, -R_ji [v~]x
            x = pick9(X, r * 3 + c);
        } else if (bj == 1) x = bi == 1 ? pick9(Rji, r * 3 + c) : 0.0;
        else x = bi == 1 ? p.dt * pick9(Rj, c * 3 + r) : (bi == 2 ? pick9(Rj, c * 3 + r) : 0.0);
    } else {
        const int cb = j - 9;
        const V3 h = v3(sH[(bi * 3 + 0) * 6 + cb], sH[(bi * 3 + 1) * 6 + cb], sH[(bi * 3 + 2) * 6 + cb]);
        x = vget(bi == 0 ? mul(so3_jr(p.tht), h) : mul(Rji, h), r);
    }
    return x;
}
__global__ void __launch_bounds__(256) k_propagate(View v, const int* __restrict__ off, const double* __restrict__ steps, ImuCov prm,
                                                  int with_cov, int from_estimate, const double* __restrict__ sig,
                                                  const int* __restrict__ sig_failed, double* __restrict__ out) {
    const int w = blockIdx.x, tid = threadIdx.x;
    if (w >= v.B) return;
    __shared__ double sF[225], sP[225], sT[225], sS[225], sA[225], sH[54], sHn[54];
    const int i = tid / 15, j = tid - i * 15;          // entry of the 15x15 matrices (tid < 225)
    double* o = out + (size_t)w * (16 + 225);
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int hi_w = v.hi[w], lo_w = v.lo[w];
    if (hi_w <= lo_w || hi_w > v.M) {                  // empty window: nothing to start from
        if (tid < 241) o[tid] = qnan;
        return;
    }
    const long gk = (long)w * v.M + hi_w - 1;
    const int b = v.sel[w], bs = from_estimate ? b ^ 1 : b;
    const bool cov_nan = with_cov && sig_failed[w] != 0;
    const double* sg = with_cov ? sig + (size_t)gk * SIG_SLOT : nullptr;
    const int s0 = off[w], s1 = off[w + 1];
    if (s1 <= s0) {
        if (tid < 16) o[tid] = XS(bs, tid, gk);
        if (tid < 225) o[16 + tid] = !with_cov || cov_nan ? qnan : sg[i >= j ? h_tri(i, j) : h_tri(j, i)];
        return;
    }
    double bh[6];
#pragma unroll
    for (int c = 0; c < 6; c++) bh[c] = XS(b, 10 + c, gk);
    const V3 bacc = v3(bh[0], bh[1], bh[2]), bgyr = v3(bh[3], bh[4], bh[5]);
    const PropMean pm = prop_integrate(steps, s0, s1, bacc, bgyr, prm, sF, sP, sT, sH, sHn);
    // (b) the state (b_i - bhat is zero unless from_estimate)
    const State si = load_state(v, bs, gk);
    const ImuPrediction p = prop_predict(v, si, pm, bh, sH);
    const State sj = predicted_state(si, p);
    if (tid == 0) {
        o[0] = sj.q.w; o[1] = sj.q.x; o[2] = sj.q.y; o[3] = sj.q.z;
        o[4] = sj.t.x; o[5] = sj.t.y; o[6] = sj.t.z;
        o[7] = sj.vel.x; o[8] = sj.vel.y; o[9] = sj.vel.z;
        o[10] = sj.ba.x; o[11] = sj.ba.y; o[12] = sj.ba.z;
        o[13] = sj.bg.x; o[14] = sj.bg.y; o[15] = sj.bg.z;
    }
    if (!with_cov || cov_nan) {                                 // (uniform over the workgroup)
        if (tid < 225) o[16 + tid] = qnan;
        return;
    }
    // (c) A (DESIGN.md "K1" at r_theta = 0) into sA, Sigma_ii into sS
    if (tid < 225) {
        sA[tid] = prop_A_entry(sj, p, sH, i, j);
        sS[tid] = sg[i >= j ? h_tri(i, j) : h_tri(j, i)];
    }
    __syncthreads();
    if (tid < 225) {
        double a = 0.0;
        for (int l = 0; l < 15; l++) a = fma(sA[i * 15 + l], sS[l * 15 + j], a);
        sT[tid] = a;
    }
    __syncthreads();
    if (tid < 225) {
        double a = 0.0;
        for (int l = 0; l < 15; l++) a = fma(sT[i * 15 + l], sA[j * 15 + l], a);
        sF[tid] = a + sP[tid];
    }
    __syncthreads();
    // B^-1 ( . ) B^-T: the velocity rows, then the velocity columns, by R_j
    const M3 Rj = qrot(sj.q);
    if (tid < 225) {
        double a = sF[tid];
        if (i >= 6 && i < 9) {
            a = 0.0;
            for (int l = 0; l < 3; l++) a = fma(pick9(Rj, (i - 6) * 3 + l), sF[(6 + l) * 15 + j], a);
        }
        sT[tid] = a;
    }
    __syncthreads();
    if (tid < 225) {
        double a = sT[tid];
        if (j >= 6 && j < 9) {
            a = 0.0;
            for (int l = 0; l < 3; l++) a = fma(sT[i * 15 + 6 + l], pick9(Rj, (j - 6) * 3 + l), a);
        }
        sS[tid] = a;
    }
    __syncthreads();
    if (tid < 225) o[16 + tid] = 0.5 * (sS[i * 15 + j] + sS[j * 15 + i]);
}
void launch_propagate(const View& v, const int* off, const double* steps, const ImuCov& prm, int with_cov, int from_estimate,
                      const double* sig, const int* sig_failed, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_propagate, dim3(v.B), dim3(256), 0, s, v, off, steps, prm, with_cov, from_estimate, sig, sig_failed, out);
}
