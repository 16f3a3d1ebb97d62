// kernels/kerr.inc -- per-factor chi-square errors of the current buffer's residuals, a summary per window, the batch's health.
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
//
// The counterpart of factor->error(values), graph.error(values) and printErrors (no reference code: the reference never asks).
// Nothing is linearised here: the whitened residuals K1, K2, K2b and the far linearisation left are read as they lie -- the bytes
// k_decide sums into cost[w] -- and the terms it throws away are kept.  Whether those residuals are of the current states is the
// engine's to know (SolveMemory::residuals_vouched); the kernels write only the buffers of FactorErrors.
// ------------------------------------------------------------------------------------ errors
// what a thread, a wave, a window knows about one class of factors; empty: max -1, argmax -1
struct ErrAcc {
    double sum, mx;
    int cnt, arg, flg, nonf;
};
VF_DI ErrAcc err_none() { return ErrAcc{0.0, -1.0, 0, -1, 0, 0}; }
// one factor's error into its class (thr: +inf where nothing is to be flagged).  An error that is not finite is counted and
// otherwise left out.  Callers visit a class in increasing index, so the strict comparison keeps the lowest index of a tie.
VF_DI void err_take(ErrAcc& a, double e, int idx, double thr) {
    a.cnt += 1;
    if (!isfinite(e)) { a.nonf += 1; return; }
    a.sum += e;
    if (e > a.mx) { a.mx = e; a.arg = idx; }
    if (2.0 * e > thr) a.flg += 1;
}
// b into a: sums add, the larger maximum wins, the lower index where they are equal (an empty side has index -1 and loses)
VF_DI void err_merge(ErrAcc& a, const ErrAcc& b) {
    a.sum += b.sum;
    a.cnt += b.cnt;
    a.flg += b.flg;
    a.nonf += b.nonf;
    if (b.arg >= 0 && (b.mx > a.mx || (b.mx == a.mx && (a.arg < 0 || b.arg < a.arg)))) { a.mx = b.mx; a.arg = b.arg; }
}
// lane 0 of the wave ends with the wave's accumulator: six shuffle steps, the same pairs whatever the data
VF_DI void err_wave_reduce(ErrAcc& a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ErrAcc b;
        b.sum = __shfl_down(a.sum, off, 64);
        b.mx = __shfl_down(a.mx, off, 64);
        b.cnt = __shfl_down(a.cnt, off, 64);
        b.arg = __shfl_down(a.arg, off, 64);
        b.flg = __shfl_down(a.flg, off, 64);
        b.nonf = __shfl_down(a.nonf, off, 64);
        err_merge(a, b);
    }
}

// Block = window, 256 threads (1024 where k_decide takes 1024), lane = keyframe slot: the rows of imu_r and btw_out are the
// coalesced AoSoA reads of k_decide, the two error arrays coalesced 8-byte stores.  Reduction per class: shuffles within a wave,
// then the waves' results through LDS in wave order -- a fixed shape, no atomics: every output is bitwise reproducible for a
// given engine.
__global__ void __launch_bounds__(1024) k_factor_errors(View v, FactorErrors o) {
    const int w = blockIdx.x, tid = threadIdx.x, nt = (int)blockDim.x;
    const int lo = v.lo[w], hi = v.hi[w], b = v.sel[w];
    const size_t tiles = (size_t)(v.G >> 6);
    const double* imu_r = v.imu_r + (size_t)b * tiles * IMU_R * TILE;
    const double* btw_out = v.btw_out + (size_t)b * tiles * BTW_OUT * TILE;
    // slots that hold no factor of this window: everything but (lo, hi)
    for (int k = tid; k < v.M; k += nt)
        if (k <= lo || k >= hi) {
            const long gk = (long)w * v.M + k;
            o.imu[gk] = -1.0;
            o.btw[gk] = -1.0;
        }
    ErrAcc ai = err_none(), ab = err_none();
    for (int k = lo + 1 + tid; k < hi; k += nt) {
        const long gk = (long)w * v.M + k;
        const double* f = imu_r + (size_t)(gk >> 6) * IMU_R * TILE + (gk & 63);
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < 15; r++) { const double x = f[(size_t)r * TILE]; c = fma(x, x, c); }
        const double ei = 0.5 * c;
        err_take(ai, ei, k, o.thr[ERR_IMU]);
        double eb = -1.0;
        const int a = v.btw_a[gk];
        if (a >= lo && a < k) {
            const double* fb = btw_out + (size_t)(gk >> 6) * BTW_OUT * TILE + (gk & 63);
            double cb = 0.0;
#pragma unroll
            for (int r = 0; r < 6; r++) { const double x = fb[(size_t)r * TILE]; cb = fma(x, x, cb); }
            eb = 0.5 * cb;
            err_take(ab, eb, k, o.thr[ERR_BETWEEN]);
        }
        o.imu[gk] = ei;
        o.btw[gk] = eb;
    }
    __shared__ ErrAcc part[2][16];
    err_wave_reduce(ai);
    err_wave_reduce(ab);
    if ((tid & 63) == 0) { part[0][tid >> 6] = ai; part[1][tid >> 6] = ab; }
    __syncthreads();
    if (tid != 0) return;
    ErrAcc cls[ERR_CLASSES];
    for (int c = 0; c < ERR_CLASSES; c++) cls[c] = err_none();
    for (int q = 0; q < (nt >> 6); q++) { err_merge(cls[ERR_IMU], part[0][q]); err_merge(cls[ERR_BETWEEN], part[1][q]); }
    // the window's own factors, as k_decide takes them
    const int pk = v.prior_k[w];
    if (pk >= lo && pk < hi) {
        const double* f = v.prior_out + ((size_t)b * v.B + w) * PRIOR_OUT;
        double c = 0.0;
        for (int r = 0; r < 15; r++) c = fma(f[r], f[r], c);
        err_take(cls[ERR_PRIOR], 0.5 * c, pk, o.thr[ERR_PRIOR]);
    }
    if (v.mp_on[w] && hi - lo >= 3) err_take(cls[ERR_MARGINAL], v.mp_out[((size_t)b * v.B + w) * 28 + 27], lo, o.thr[ERR_MARGINAL]);
    // far factors: alive as the far lists say (vf_far.hpp), not "the words are not zero"
    double* far = o.far + (size_t)w * 2 * o.x_cap;
    for (int s = 0; s < 2 * o.x_cap; s++) far[s] = -1.0;
    if (v.x_max > 0) {
        const int nl = v.xl_n[w];
        for (int i = 0; i < v.x_max; i++) {                     // entry i of the window's list of nonlinear far factors
            const FarRef f = far_ref(v, w, nl + i);
            if (f.kind != 0) continue;
            double c = 0.0;
            for (int r = 0; r < 6; r++) { const double x = far_res(v, w, f, b, r); c = fma(x, x, c); }
            far[i] = 0.5 * c;
            err_take(cls[ERR_FAR], far[i], i, o.thr[ERR_FAR]);
        }
        for (int s = 0; s < nl && s < v.x_max; s++) {           // far end s of the window's linear far factor
            const FarRef f = far_ref(v, w, s);
            if (f.kind != 1) continue;
            double c = 0.0;
            for (int r = 0; r < 6; r++) { const double x = far_res(v, w, f, b, r); c = fma(x, x, c); }
            far[o.x_cap + s] = 0.5 * c;
            err_take(cls[ERR_FAR_LINEAR], far[o.x_cap + s], s, o.thr[ERR_FAR_LINEAR]);
        }
    }
    ErrSummary s;
    s.reserved0 = 0;
    s.status = 0;
    s.total = 0.0;
    s.rows = 0;
    const int rows_of[ERR_CLASSES] = {15, 6, 15, 27, 6, 6};
    for (int c = 0; c < ERR_CLASSES; c++) {
        s.count[c] = cls[c].cnt;
        s.argmax[c] = cls[c].arg;
        s.flagged[c] = cls[c].flg;
        s.nonfinite[c] = cls[c].nonf;
        s.sum[c] = cls[c].sum;
        s.max[c] = cls[c].mx;
        s.total += cls[c].sum;
        s.rows += rows_of[c] * cls[c].cnt;
        if (cls[c].nonf) s.status |= ERR_STATUS_NONFINITE;
        if (cls[c].flg) s.status |= ERR_STATUS_FLAGGED;
    }
    s.keyframes = hi > lo ? hi - lo : 0;
    s.unknowns = 15 * s.keyframes;
    s.reserved1 = 0;
    if (hi <= lo) s.status |= ERR_STATUS_EMPTY;
    o.summary[w] = s;
}

// One workgroup over the windows' summaries and the LM words (the lifetime counters vf_engine_read_lm returns): counts, and the
// window with the largest reduced chi-square 2 total / max(rows - unknowns, 1), the lowest index of a tie.  Integer sums and a
// maximum with a tie rule: the same whatever the order.
__global__ void __launch_bounds__(256) k_batch_health(View v, FactorErrors o) {
    const int tid = threadIdx.x;
    int empty = 0, failed = 0, nonf = 0, never = 0, flagged = 0, worst = -1;
    double wv = 0.0;
    for (int w = tid; w < v.B; w += 256) {
        const ErrSummary& s = o.summary[w];
        const bool is_empty = (s.status & ERR_STATUS_EMPTY) != 0;
        empty += is_empty;
        failed += v.n_fail[w] > 0;
        nonf += !isfinite(v.cost[w]) || (s.status & ERR_STATUS_NONFINITE) != 0;
        never += !is_empty && v.n_acc[w] == 0;
        flagged += (s.status & ERR_STATUS_FLAGGED) != 0;
        if (is_empty) continue;
        const int dof = s.rows - s.unknowns;
        const double x = 2.0 * s.total / (double)(dof > 1 ? dof : 1);
        if (worst < 0 || x > wv) { worst = w; wv = x; }
    }
    __shared__ int cnt[5][256], wi[256];
    __shared__ double wx[256];
    cnt[0][tid] = empty; cnt[1][tid] = failed; cnt[2][tid] = nonf; cnt[3][tid] = never; cnt[4][tid] = flagged;
    wi[tid] = worst;
    wx[tid] = wv;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            for (int c = 0; c < 5; c++) cnt[c][tid] += cnt[c][tid + st];
            const int j = wi[tid + st];
            if (j >= 0 && (wi[tid] < 0 || wx[tid + st] > wx[tid] || (wx[tid + st] == wx[tid] && j < wi[tid]))) { wi[tid] = j; wx[tid] = wx[tid + st]; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        BatchHealth h;
        h.reserved0 = 0;
        h.windows = v.B;
        h.empty = cnt[0][0];
        h.failed = cnt[1][0];
        h.nonfinite = cnt[2][0];
        h.never_accepted = cnt[3][0];
        h.flagged_windows = cnt[4][0];
        h.worst_window = wi[0];
        h.worst_reduced_chi2 = wi[0] >= 0 ? wx[0] : 0.0;
        *o.health = h;
    }
}
void launch_factor_errors(const View& v, const FactorErrors& o, hipStream_t s) {
    hipLaunchKernelGGL(k_factor_errors, dim3(v.B), dim3(v.B <= 64 ? 1024 : 256), 0, s, v, o);       // (k_decide's launch rule)
    hipLaunchKernelGGL(k_batch_health, dim3(1), dim3(256), 0, s, v, o);
}
