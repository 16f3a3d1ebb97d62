// kernels/kclosure.inc -- the loop-closure gate: chi-square of a candidate between factor on ANY two solved keyframes of a window,
// before it is added (DESIGN.md section 4j; vf_engine_gate_closures).
// A section of vf_kernels.hip (ONE translation unit); included from there behind kgate.inc, inside namespace vf, never compiled by
// itself.
//
// The tail gate (kgate.inc) reads Cov(pose_j, pose_a) off the profile of the selected inversion and so reaches a in {i, i-1}.  Here
// the joint pose covariance of keyframes a < b anywhere in [lo, hi) comes from COLUMNS of the inverse: with E_c the six unit
// columns of the pose dofs of keyframe c,
//     Sigma_cd^pp = (A^-1 E_d)[c, 0:6] - Y_c^p (Y_d^p)^T
// A = H_band on the panels of the undamped sweep, Y = Z R^-T of the far factors alive (k4_selinv_far.inc: Z = A^-1 U, C = I + U^T Z
// = R R^T; its kernels run as they are, all but the downdate of sig).  Four kernels per group of windows:
//   k_closure_rhs      the unit entries of the window's distinct candidate keyframes into its zeroed column block
//   k_closure_forward  forward substitution on the panels, a lane per column, from the SMALLEST such keyframe k0 (the columns are
//                      exactly zero in front of it: a sweep from lo would carry zeros to k0 and arrive with the state this one starts from)
//   k_closure_back     back substitution, down to k0 (no row in front of it is read)
//   k_gate_closure     per candidate: Sigma_J (12 x 12, symmetrised), r, Ja, Jb (between_values), S, its Cholesky factor, the record
// The substitutions are those of k_farcov_forward / k_farcov_back, built from the same pieces: farcov_fetch, farcov_stage, the
// lane's 27 pending entries in LDS at [64 i + lane] (a lane's own bank: conflict-free), the next panel prefetched into registers.
// Every column is one lane's own chain of operations: a candidate's record does not depend on what else the call holds.
// Column 6 j + p of a window is pose dof p of its j-th distinct keyframe (ascending); candidates that share an end share its columns.
struct ClosureOut {              // vf_closure_gate_result's layout (CLOSURE_RECORD bytes)
    unsigned struct_size;
    int status, rejected, window, a, b;
    double nis, nis_measurement, xi[6];
};
static_assert(sizeof(ClosureOut) == CLOSURE_RECORD, "ClosureOut and CLOSURE_RECORD");

// the window's smallest column keyframe, or -1: nothing to do (no candidate to test, a failed or empty window, keys outside it)
VF_DI int closure_first(const View& v, const ClosureGate& cg, int w) {
    const int lo = v.lo[w], hi = v.hi[w], nk = cg.nkeys[w];
    if (hi - lo <= 0 || hi > v.M || lo < 0 || cg.failed[w] || nk <= 0 || nk > CLOSURE_KEYS) return -1;
    const int k0 = cg.keys[w * CLOSURE_KEYS], k1 = cg.keys[w * CLOSURE_KEYS + nk - 1];
    return k0 < lo || k1 >= hi || k0 > k1 ? -1 : k0;
}
__global__ void __launch_bounds__(64) k_closure_rhs(View v, ClosureGate cg) {
    const int w = cg.w0 + blockIdx.x, q = threadIdx.x, nc = cg.nc;
    const int k0 = closure_first(v, cg, w);
    if (q >= nc || k0 < 0) return;
    const int hi = v.hi[w];
    double* __restrict__ X = cg.X + (size_t)blockIdx.x * cg.xwin;
    for (int i = k0 * 15; i < hi * 15; i++) X[(size_t)i * nc + q] = 0.0;
    if (q < 6 * cg.nkeys[w]) {
        const int k = cg.keys[w * CLOSURE_KEYS + q / 6];
        if (k >= k0 && k < hi) X[((size_t)k * 15 + q % 6) * nc + q] = 1.0;
    }
}
__global__ void __launch_bounds__(64) k_closure_forward(View v, ClosureGate cg) {
    const int w = cg.w0 + blockIdx.x, lane = threadIdx.x, col = blockIdx.y * 64 + lane, m = cg.nc;
    const int k0 = closure_first(v, cg, w);
    if (k0 < 0) return;
    const int hi = v.hi[w];
    const bool mine = col < m;
    double* __restrict__ zc = cg.X + (size_t)blockIdx.x * cg.xwin + (mine ? col : 0);
    __shared__ FarPanel P;
    __shared__ double PS[27 * 64];       // the lane's pending updates of [k: 15][k+1: pose][k+2: pose], entry i at PS[64 i + lane]
    for (int i = 0; i < 27; i++) PS[64 * i + lane] = 0.0;
    double pf[FC_PF], nx[15];
    farcov_fetch(v, w, k0, hi, lane, pf);
#pragma unroll
    for (int d = 0; d < 15; d++) nx[d] = mine ? zc[((size_t)k0 * 15 + d) * m] : 0.0;
#pragma unroll 1
    for (int k = k0; k < hi; k++) {
        farcov_stage<false>(P, lane, pf);
        __syncthreads();
        if (k + 1 < hi) farcov_fetch(v, w, k + 1, hi, lane, pf);
        double r[15], y[15];
#pragma unroll
        for (int d = 0; d < 15; d++) r[d] = nx[d] - PS[64 * d + lane];
        double* __restrict__ zk = zc + (size_t)k * 15 * m;
#pragma unroll
        for (int j = 0; j < 15; j++) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i <= j; i++) s = fma(P.PU[j * SI_LD + i], r[i], s);     // U^T[j][i], zero for i > j
            y[j] = s;
        }
        if (mine)
#pragma unroll
            for (int d = 0; d < 15; d++) zk[d * m] = y[d];
        if (k + 1 < hi && mine)
#pragma unroll
            for (int d = 0; d < 15; d++) nx[d] = zk[(15 + d) * m];
        // pending of k + 1, as k_farcov_forward forms it: every old row is read before it is overwritten
#pragma unroll 3
        for (int i = 0; i < 27; i++) {
            double s = i < 6 ? PS[64 * (15 + i) + lane] : (i >= 15 && i < 21 ? PS[64 * (i + 6) + lane] : 0.0);
#pragma unroll
            for (int j = 0; j < 15; j++) s = fma(P.PB[i * SI_LD + j], y[j], s);
            PS[64 * i + lane] = s;
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(64) k_closure_back(View v, ClosureGate cg) {
    const int w = cg.w0 + blockIdx.x, lane = threadIdx.x, col = blockIdx.y * 64 + lane, m = cg.nc;
    const int k0 = closure_first(v, cg, w);
    if (k0 < 0) return;
    const int hi = v.hi[w];
    const bool mine = col < m;
    double* __restrict__ zc = cg.X + (size_t)blockIdx.x * cg.xwin + (mine ? col : 0);
    __shared__ FarPanel P;
    __shared__ double XS[27 * 64];       // the lane's x_S: [k+1: 15][k+2: pose][k+3: pose], entry i at XS[64 i + lane]
    for (int i = 0; i < 27; i++) XS[64 * i + lane] = 0.0;
    double pf[FC_PF], nx[15];
    farcov_fetch(v, w, hi - 1, hi, lane, pf);
#pragma unroll
    for (int d = 0; d < 15; d++) nx[d] = mine ? zc[((size_t)(hi - 1) * 15 + d) * m] : 0.0;
#pragma unroll 1
    for (int k = hi - 1; k >= k0; k--) {
        farcov_stage<true>(P, lane, pf);
        __syncthreads();
        if (k > k0) farcov_fetch(v, w, k - 1, hi, lane, pf);
        double t[15];
#pragma unroll
        for (int j = 0; j < 15; j++) {
            double s = nx[j];
#pragma unroll 9
            for (int i = 0; i < 27; i++) s = fma(-P.PB[j * FC_BT + i], XS[64 * i + lane], s);
            t[j] = s;
        }
        double* __restrict__ zk = zc + (size_t)k * 15 * m;
        // x_S of k - 1: the pose rows of k+1 move down first (each lane its own column)
#pragma unroll
        for (int i = 0; i < 6; i++) { XS[64 * (21 + i) + lane] = XS[64 * (15 + i) + lane]; XS[64 * (15 + i) + lane] = XS[64 * i + lane]; }
#pragma unroll
        for (int i = 0; i < 15; i++) {
            double s = 0.0;
#pragma unroll
            for (int j = i; j < 15; j++) s = fma(P.PU[i * SI_LD + j], t[j], s);
            XS[64 * i + lane] = s;
            if (mine) zk[i * m] = s;
        }
        if (k > k0 && mine)
#pragma unroll
            for (int d = 0; d < 15; d++) nx[d] = zk[(d - 15) * m];
        __syncthreads();
    }
}
// One 128-thread workgroup per window.  First thread c takes candidate c (at most CLOSURE_MAX): its status, its columns, and r, Ja,
// Jb, xi at the current buffer's T_a, T_b into LDS; then the workgroup goes through the candidates one after the other: Y rows,
// Sigma_J, S, nis.  Writes the candidate's record and the 144 doubles of Sigma_J (NaN unless the candidate was tested) into the
// call's buffers, nothing else.
constexpr int CG_NT = 128;
__global__ void __launch_bounds__(CG_NT) k_gate_closure(View v, ClosureGate cg, FarCov fc) {
    extern __shared__ double ylds[];                   // [12][m + 1]: the pose rows of Y_a, Y_b (far factors alive only)
    __shared__ double sJ[CLOSURE_MAX][72], sR[CLOSURE_MAX][6], sXi[CLOSURE_MAX][6], sJoint[144], sM[144], sU[72], sSm[36];
    __shared__ int sStatus[CLOSURE_MAX], sCol[CLOSURE_MAX][2];
    const int w = cg.w0 + blockIdx.x, tid = threadIdx.x;
    if (w >= v.B) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int ncand = min(cg.cnt[w], CLOSURE_MAX);
    const int lo = v.lo[w], hi = v.hi[w];
    const bool range_ok = hi - lo > 0 && hi <= v.M && lo >= 0, failed = cg.failed[w] != 0;
    if (tid < ncand) {
        const int ci = cg.idx[w * CLOSURE_MAX + tid], a = cg.a[ci], b = cg.b[ci];
        int status = cg.status[ci], ja = -1, jb = -1;
        if (status == GATE_OK) {
            const int nk = min(cg.nkeys[w], CLOSURE_KEYS);
            for (int j = 0; j < nk; j++) {
                const int k = cg.keys[w * CLOSURE_KEYS + j];
                if (k == a) ja = j;
                if (k == b) jb = j;
            }
            // (the device's own range decides; a failed window is answered with the innovation alone)
            if (!range_ok || a < lo || a >= b || b >= hi || ja < 0 || jb < 0 || (!failed && closure_first(v, cg, w) < 0)) status = GATE_OUT_OF_REACH;
        }
        sStatus[tid] = status;
        sCol[tid][0] = ja;
        sCol[tid][1] = jb;
        if (status == GATE_OK) {
            const int sel = cg.from_estimate ? v.sel[w] ^ 1 : v.sel[w];      // (the trial buffer: the estimate of a reference-compat engine)
            const long ga = (long)w * v.M + a, gb = (long)w * v.M + b;
            const Q4 qa = q4(XS(sel, 0, ga), XS(sel, 1, ga), XS(sel, 2, ga), XS(sel, 3, ga));
            const V3 ta = v3(XS(sel, 4, ga), XS(sel, 5, ga), XS(sel, 6, ga));
            const Q4 qb = q4(XS(sel, 0, gb), XS(sel, 1, gb), XS(sel, 2, gb), XS(sel, 3, gb));
            const V3 tb = v3(XS(sel, 4, gb), XS(sel, 5, gb), XS(sel, 6, gb));
            const double* __restrict__ rec = cg.rec + (size_t)ci * BTW_IN;
            GateSink sink{sJ[tid], sR[tid]};
            const Xi6 xi = between_values(qa, ta, qb, tb, [rec](int f) { return rec[f]; }, sink);
            sXi[tid][0] = xi.w.x; sXi[tid][1] = xi.w.y; sXi[tid][2] = xi.w.z; sXi[tid][3] = xi.u.x; sXi[tid][4] = xi.u.y; sXi[tid][5] = xi.u.z;
        }
    }
    __syncthreads();
    const int nc = cg.nc, m = fc.m, ld = m + 1;
    const bool far = m > 0 && range_ok && far_live(v, w, fc.slots);
    const double* __restrict__ X = cg.X + (size_t)blockIdx.x * cg.xwin;
    const double* __restrict__ Z = fc.Z + (size_t)blockIdx.x * fc.zwin;
    const double* __restrict__ R = fc.C + (size_t)blockIdx.x * fc.cwin;
#pragma unroll 1
    for (int c = 0; c < ncand; c++) {
        const int ci = cg.idx[w * CLOSURE_MAX + c];
        const int a = cg.a[ci], b = cg.b[ci], status = sStatus[c], ja = sCol[c][0], jb = sCol[c][1];
        ClosureOut* o = (ClosureOut*)(cg.out + (size_t)ci * CLOSURE_RECORD);
        double* __restrict__ jo = cg.joint + (size_t)ci * 144;
        if (tid == 0) { o->struct_size = 0; o->window = w; o->a = a; o->b = b; }
        if (status != GATE_OK || failed) {
            // nothing to test; or the factorisation, or the far system C, failed: the innovation without its covariance
            for (int e = tid; e < 144; e += CG_NT) jo[e] = qnan;
            if (tid < 6) o->xi[tid] = status == GATE_OK ? sXi[c][tid] : qnan;
            if (tid == 0) {
                double mm = 0.0;
                for (int r = 0; r < 6; r++) mm = fma(sR[c][r], sR[c][r], mm);
                o->status = status == GATE_OK ? GATE_NO_COVARIANCE : status;
                o->rejected = 0;
                o->nis = qnan;
                o->nis_measurement = status == GATE_OK ? mm : qnan;
            }
            continue;
        }
        if (far) {
            // Y rows = Z rows solved against R in place, a thread per row, by k_farcov_downdate's chain
            for (int e = tid; e < 12 * m; e += CG_NT) {
                const int i = e / m, q = e - (e / m) * m;
                ylds[i * ld + q] = Z[((size_t)(i < 6 ? a : b) * 15 + (i < 6 ? i : i - 6)) * m + q];
            }
            __syncthreads();
            if (tid < 12) {
                double* __restrict__ y = ylds + tid * ld;
                for (int p = 0; p < m; p++) {
                    double s = y[p];
                    for (int q = 0; q < p; q++) s = fma(-R[p * m + q], y[q], s);
                    y[p] = s / R[p * m + p];
                }
            }
            __syncthreads();
        }
        for (int e = tid; e < 144; e += CG_NT) {
            const int r = e / 12, cc = e - 12 * r;
            const int kr = r < 6 ? a : b, ir = r < 6 ? r : r - 6, jc = cc < 6 ? ja : jb, pc = cc < 6 ? cc : cc - 6;
            double x = X[((size_t)kr * 15 + ir) * nc + 6 * jc + pc];
            if (far) {
                double s = 0.0;
                for (int q = 0; q < m; q++) s = fma(ylds[r * ld + q], ylds[cc * ld + q], s);
                x -= s;
            }
            sM[e] = x;
        }
        __syncthreads();
        for (int e = tid; e < 144; e += CG_NT) {
            const int r = e / 12, cc = e - 12 * r;
            const double x = 0.5 * (sM[r * 12 + cc] + sM[cc * 12 + r]);
            sJoint[e] = x;
            jo[e] = x;
        }
        __syncthreads();
        double nis, mm;
        const bool spd = gate_nis(tid, sJ[c], sR[c], sJoint, sU, sSm, nis, mm);
        if (tid < 6) o->xi[tid] = sXi[c][tid];
        if (tid == 0) {
            o->status = spd ? GATE_OK : GATE_NO_COVARIANCE;
            o->rejected = spd && nis > cg.threshold ? 1 : 0;
            o->nis = spd ? nis : qnan;
            o->nis_measurement = mm;
        }
        __syncthreads();                               // (the next candidate overwrites sJoint, sM, ylds)
    }
}
void launch_closure_gate(const View& v, const ClosureGate& cg, const FarCov& fc, int nw, hipStream_t s) {
    const unsigned cb = (unsigned)((cg.nc + 63) / 64);
    if (cg.nc > 0) {
        hipLaunchKernelGGL(k_closure_rhs, dim3((unsigned)nw), dim3(64), 0, s, v, cg);
        hipLaunchKernelGGL(k_closure_forward, dim3((unsigned)nw, cb), dim3(64), 0, s, v, cg);
        hipLaunchKernelGGL(k_closure_back, dim3((unsigned)nw, cb), dim3(64), 0, s, v, cg);
    }
    if (fc.m > 0) launch_farcov_system(v, fc, nw, s);
    hipLaunchKernelGGL(k_gate_closure, dim3((unsigned)nw), dim3(CG_NT), (size_t)12 * (fc.m + 1) * sizeof(double), s, v, cg, fc);
}
