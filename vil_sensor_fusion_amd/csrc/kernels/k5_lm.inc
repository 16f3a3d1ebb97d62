// kernels/k5_lm.inc -- K5: retract, cost + LM decision, excursions; a2: prediction; relinearisation (reference-compat and incremental).
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ K5
__global__ void __launch_bounds__(256) k_retract(View v) {
    const long gk = (long)blockIdx.x * 256 + threadIdx.x;
    if (gk >= v.G) return;
    const int w = (int)(gk / v.M), k = (int)(gk - (long)w * v.M);
    if (k < v.lo[w] || k >= v.hi[w] || window_done(v, w)) return;
    const int b = v.sel[w];
    const State s = load_state(v, b, gk);
    const double* d = v.delta + (size_t)gk * 15;
    State o;
    Q4 dq;
    V3 dtv;
    se3_exp(v3(d[0], d[1], d[2]), v3(d[3], d[4], d[5]), &dq, &dtv);
    o.q = qnormalize(qmul(s.q, dq));
    o.t = s.t + mul(qrot(s.q), dtv);
    o.vel = s.vel + v3(d[6], d[7], d[8]);
    o.ba = s.ba + v3(d[9], d[10], d[11]);
    o.bg = s.bg + v3(d[12], d[13], d[14]);
    store_state(v, b ^ 1, gk, o);
}

// The decrease of the cost that the linearised problem predicts for the increment just solved (GTSAM's linearizedCostChange,
// LevenbergMarquardtOptimizer::tryLambda): 0.5 |r|^2 - 0.5 |r + J d|^2 = -g.d - 0.5 d^T H d, and with (H + lambda I) d = -g that is
// 0.5 (lambda |d|^2 - g.d): two dot products over the window, fixed-shape reduction.  Needs g in HBM: engines that use this
// rule run K3 (the assembling sweep keeps g in LDS).
__global__ void __launch_bounds__(256) k_model_change(View v) {
    const int w = blockIdx.x, tid = threadIdx.x;
    if (window_done(v, w)) return;
    const int lo = v.lo[w], hi = v.hi[w];
    double gd = 0.0, dd = 0.0;
    for (int e = tid; e < (hi - lo) * 15; e += 256) {
        const size_t o = ((size_t)w * v.M + lo) * 15 + e;
        const double d = v.delta[o];
        gd = fma(v.gvec[o], d, gd);
        dd = fma(d, d, dd);
    }
    __shared__ double r0[256], r1[256];
    r0[tid] = gd;
    r1[tid] = dd;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) { r0[tid] += r0[tid + st]; r1[tid] += r1[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) v.model[w] = 0.5 * (v.lambda[w] * r1[0] - r0[0]);
}

// cost of buffer (sel ^ !init) per window, then the LM decision.  Block = window, 256 threads (1024 when there are few
// windows: the per-thread loop over a long window's factors is a latency chain); fixed-shape tree reduction, so the
// cost is bitwise reproducible for a given engine.
// Time-sharded windows: every rank holds the residual of every factor (k_linearize_all<true>), so every rank forms the
// whole cost itself and takes the same decision -- no exchange; the solve-failure flags of the other ranks arrive in the
// tail of the increment buffer, summed by the same all-reduce as the increments (k_mask_delta).
__global__ void __launch_bounds__(1024) k_decide(View v, int init) {
    const int w = blockIdx.x, tid = threadIdx.x;
    if (window_done(v, w) && !init) return;
    const int lo = v.lo[w], hi = v.hi[w];
    const int b = init ? v.sel[w] : (v.sel[w] ^ 1);
    const size_t tiles = (size_t)(v.G >> 6);
    const double* imu_r = v.imu_r + (size_t)b * tiles * IMU_R * TILE;
    const double* btw_out = v.btw_out + (size_t)b * tiles * BTW_OUT * TILE;
    double s = 0.0;
    const int nt = (int)blockDim.x;
    for (int k = lo + 1 + tid; k < hi; k += nt) {
        const long gk = (long)w * v.M + k;
        const double* f = imu_r + (size_t)(gk >> 6) * IMU_R * TILE + (gk & 63);
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < 15; r++) { const double x = f[(size_t)r * TILE]; c = fma(x, x, c); }
        const int a = v.btw_a[gk];
        if (a >= lo && a < k) {
            const double* fb = btw_out + (size_t)(gk >> 6) * BTW_OUT * TILE + (gk & 63);
#pragma unroll
            for (int r = 0; r < 6; r++) { const double x = fb[(size_t)r * TILE]; c = fma(x, x, c); }
        }
        s += c;
    }
    if (tid == 0) {
        const int pk = v.prior_k[w];
        if (pk >= lo && pk < hi) {
            const double* f = v.prior_out + ((size_t)b * v.B + w) * PRIOR_OUT;
            for (int r = 0; r < 15; r++) s = fma(f[r], f[r], s);
        }
        if (v.mp_on[w] && hi - lo >= 3) s += 2.0 * v.mp_out[((size_t)b * v.B + w) * 28 + 27];
        for (int xs = 0; xs < v.x_max; xs++) {           // far between factors, nonlinear and linear (empty slots hold zeros)
            const double* f = v.x_out + (((size_t)b * v.B + w) * v.x_max + xs) * BTW_OUT;
            const double* fl = v.xl_out + ((size_t)b * v.B + w) * 6 * v.x_max + 6 * xs;
            for (int r = 0; r < 6; r++) s = fma(f[r], f[r], fma(fl[r], fl[r], s));
        }
    }
    __shared__ double red[1024];
    __shared__ int outcome_s;
    red[tid] = s;
    __syncthreads();
    for (int st = nt >> 1; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    // outcome of the trial: 0 rejected, 1 accepted, 2 kept provisionally (non-monotone LM: the cost rose, the excursion goes
    // on), 3 the excursion failed (the point it started from is restored)
    if (tid == 0) {
        const double c = 0.5 * red[0];
        if (v.sh_G > 1 && !init) v.fail[w] = v.delta[(size_t)v.G * 15 + w] > 0.0 ? 1 : 0;   // a failed elimination on any rank rejects the trial
        if (init) {
            v.cost[w] = c;
            v.fail[w] = 0;
            if (!(v.fresh[w] >= 2 && v.fresh[w] < 64)) v.fresh[w] = 1;   // (a warm start has marked the window "ends only")
            if (v.stop_on) v.done[w] = 0;
            if (v.nm_W > 0) v.prov[w] = 0;
            outcome_s = -1;
        } else {
            // accept unless the cost rises by more than the rounding floor of its own evaluation (View::accept_rel): at a
            // converged window a strict "c < cost" is decided by the last bits of two 1000-term sums, and a rejected
            // Newton step leaves the soft modes of the window where they were (DESIGN.md "Accept rule at the floor")
            const int prov = v.nm_W > 0 ? v.prov[w] : 0;
            const double refc = prov > 0 ? v.ref_cost[w] : v.cost[w];        // an excursion is judged against the point it left
            const bool solved = v.fail[w] == 0;
            bool ok = solved && (c < refc + v.accept_rel * refc);
            if (v.min_fidelity > 0.0) {       // GTSAM: modelFidelity = costChange / linearizedCostChange > minModelFidelity
                const double predicted = v.model[w];
                ok = solved && predicted > 0.0 && (refc - c) > v.min_fidelity * predicted;
            }
            const int outcome = ok ? 1 : (v.nm_W > 0 && solved && prov < v.nm_W) ? 2 : (prov > 0 ? 3 : 0);
            outcome_s = outcome | (prov << 8);
            if (!solved) v.n_fail[w] += 1;
            v.fresh[w] = outcome ? 1 : 0;
            if (v.stop_on && solved && outcome < 2) {
                // gtsam checkConvergence (absolute / relative decrease of the accepted step), applied to rejected
                // trials too: a trial that changes the cost by less than the tolerance in either direction means
                // the window sits at its rounding floor, where accept / reject is decided by the last bit
                const double dec = fabs(refc - c);
                if (dec <= v.abs_tol || dec <= v.rel_tol * refc) v.done[w] = 1;
            }
            double l = v.lambda[w];
            if (outcome == 1 || outcome == 2) {
                if (outcome == 2 && prov == 0) v.ref_cost[w] = v.cost[w];
                v.sel[w] ^= 1;
                v.cost[w] = c;
                if (outcome == 1) v.n_acc[w] += 1; else v.n_prov[w] += 1;
                // (a provisional trial divides twice: an excursion is the damped iteration's way towards the Gauss-Newton
                // step, whose cost falls only once the stiff residuals its first-order move disturbed have been corrected)
                l = outcome == 1 ? l / v.lam_down : l / (v.lam_down * v.lam_down);
                v.lambda[w] = l < v.lam_min ? v.lam_min : l;
                if (v.nm_W > 0) v.prov[w] = outcome == 1 ? 0 : prov + 1;
            } else {
                v.n_rej[w] += 1;
                l *= v.lam_up;
                v.lambda[w] = l > v.lam_max ? v.lam_max : l;
                if (outcome == 3) { v.cost[w] = refc; v.prov[w] = 0; v.relin[w] = 1; }
            }
            v.fail[w] = 0;
        }
    }
    if (v.nm_W > 0 && !init) {
        __syncthreads();
        const int outcome = outcome_s & 0xff, prov = outcome_s >> 8;
        // (v.sel[w] was read into b = sel ^ 1 at the top: b ^ 1 is the buffer that was current when the trial was made)
        if (outcome == 2 && prov == 0)
            for (int e = tid; e < (hi - lo) * 16; e += nt) {
                const int cc = e / (hi - lo), k = lo + e - cc * (hi - lo);
                v.x_best[(size_t)cc * v.G + (size_t)w * v.M + k] = XS(b ^ 1, cc, (long)w * v.M + k);
            }
        if (outcome == 3)
            for (int e = tid; e < (hi - lo) * 16; e += nt) {
                const int cc = e / (hi - lo), k = lo + e - cc * (hi - lo);
                XS(b ^ 1, cc, (long)w * v.M + k) = v.x_best[(size_t)cc * v.G + (size_t)w * v.M + k];
            }
    }
}

// non-monotone LM, end of a solve: an excursion still open when the trials run out is undone (the point it started from was
// the best one seen)
__global__ void __launch_bounds__(1024) k_close_excursion(View v) {
    const int w = blockIdx.x, tid = threadIdx.x, nt = (int)blockDim.x;
    const int prov = v.prov[w], lo = v.lo[w], hi = v.hi[w], b = v.sel[w];
    __syncthreads();
    if (prov <= 0 || hi - lo <= 0) return;
    for (int e = tid; e < (hi - lo) * 16; e += nt) {
        const int cc = e / (hi - lo), k = lo + e - cc * (hi - lo);
        XS(b, cc, (long)w * v.M + k) = v.x_best[(size_t)cc * v.G + (size_t)w * v.M + k];
    }
    // (carry: the next solve keeps the damping the excursion had reached instead of starting from lambda0 again -- k_reset_lambda --
    // or a window that needs more trials than one solve has would repeat the same first trials for ever.  The host marks EVERY
    // window of an engine that runs excursions behind this kernel, vf_engine_close_excursions: this store alone would carry
    // only the windows cut off inside an excursion)
    if (tid == 0) { v.cost[w] = v.ref_cost[w]; v.prov[w] = 0; v.relin[w] = 1; v.fresh[w] = 1; v.carry[w] = 1; }
}
// every solve starts from lambda0, as a fresh LevenbergMarquardtOptimizer would -- except on an engine that runs non-monotone LM
// (lm_excursion > 0): there every window goes on from the damping its previous solve ended with, whether or not that solve was cut
// off inside an excursion (vf_engine_close_excursions sets carry[] for all windows; include/vilfusion.h "lambda PERSISTS";
// tests/test_gpu_lm_trace.py::test_damping_carries_between_solves)
// (clear_done: a warm solve's "no window is converged yet" rides along -- one launch less in front of k_linearize_tail)
__global__ void __launch_bounds__(256) k_reset_lambda(View v, const double* __restrict__ lambda0, int clear_done) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= v.B) return;
    if (clear_done) v.done[w] = 0;
    if (v.carry && v.carry[w]) { v.carry[w] = 0; return; }
    v.lambda[w] = lambda0[w];
}

// ------------------------------------------------------------------------------------ a2
VF_DI State predict_state(const View& v, const State& si, long gk_factor) {
    const ImuRecordHbm rec = {v.imu_in + (size_t)(gk_factor >> 6) * IMU_IN * TILE + (gk_factor & 63)};
    return predicted_state(si, imu_predict(v, si, rec));
}

// window < 0: all windows (one lane each)
// from_trial: the first prediction starts from the TRIAL buffer's state of keyframe k0 - 1 (reference-compat solves: the
// trial buffer holds the estimate theta (+) delta the reference predicts from, GraphManager.cpp:152-153)
__global__ void k_predict(View v, int window, int k0, int n, int from_trial) {
    const int w = window >= 0 ? window : (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w >= v.B || (window >= 0 && (blockIdx.x | threadIdx.x))) return;
    const int b = v.sel[w];
    for (int k = k0; k < k0 + n; k++) {
        const long gk = (long)w * v.M + k;
        const State si = load_state(v, (from_trial && k == k0) ? b ^ 1 : b, gk - 1);
        const State sn = predict_state(v, si, gk);
        store_state(v, b, gk, sn);
        if (from_trial) store_state(v, b ^ 1, gk, sn);      // the estimate of a keyframe that has no increment yet
    }
}

// Reference-compat solves (one iSAM2-like update per vf_solve, GraphManager.cpp:38-43,126-127): fluid relinearisation --
// a keyframe whose pending increment reaches the threshold in any component (ISAM2Params::relinearizeThreshold, a scalar:
// max |delta| >= threshold) moves its linearisation point there, theta <- theta (+) delta, delta <- 0; the others keep
// theirs.  Lane = keyframe.
__global__ void __launch_bounds__(256) k_relinearize(View v, double threshold) {
    const long gk = (long)blockIdx.x * 256 + threadIdx.x;
    if (gk >= v.G) return;
    const int w = (int)(gk / v.M), k = (int)(gk - (long)w * v.M);
    if (k < v.lo[w] || k >= v.hi[w]) return;
    double* d = v.delta + (size_t)gk * 15;
    double m = 0.0;
#pragma unroll
    for (int a = 0; a < 15; a++) m = fmax(m, fabs(d[a]));
    if (!(m >= threshold)) return;
    const int b = v.sel[w];
    const State s = load_state(v, b, gk);
    State o;
    Q4 dq;
    V3 dtv;
    se3_exp(v3(d[0], d[1], d[2]), v3(d[3], d[4], d[5]), &dq, &dtv);
    o.q = qnormalize(qmul(s.q, dq));
    o.t = s.t + mul(qrot(s.q), dtv);
    o.vel = s.vel + v3(d[6], d[7], d[8]);
    o.ba = s.ba + v3(d[9], d[10], d[11]);
    o.bg = s.bg + v3(d[12], d[13], d[14]);
    store_state(v, b, gk, o);
#pragma unroll
    for (int a = 0; a < 15; a++) d[a] = 0.0;
}

// The same for incremental updates (View::inc_*), which also need to know WHERE the first change is: the first slot whose
// linearisation point moves here, or the first of the `appended` keyframes at the window's end (their factors are new), or
// the window's first keyframe when the caller says the factorisation is void.  Only keyframes from inc_stop on have an
// increment that the last back substitution touched.  inc_k is INT_MAX when this runs (k_inc_retract leaves it so).
__global__ void __launch_bounds__(256) k_inc_begin(View v, double threshold, int appended, int invalid) {
    const int w = blockIdx.y;
    const int lo = v.lo[w], hi = v.hi[w];
    const int from = invalid ? lo : v.inc_stop[w];
    const int k = (from & ~255) + (int)(blockIdx.x * 256 + threadIdx.x);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMin(v.inc_k + w, invalid ? lo : (hi - appended > lo ? hi - appended : lo));
    if (k < lo || k < from || k >= hi) return;
    const long gk = (long)w * v.M + k;
    double* d = v.delta + (size_t)gk * 15;
    double m = 0.0;
#pragma unroll
    for (int a = 0; a < 15; a++) m = fmax(m, fabs(d[a]));
    if (!(m >= threshold)) return;
    const int b = v.sel[w];
    const State s = load_state(v, b, gk);
    State o;
    Q4 dq;
    V3 dtv;
    se3_exp(v3(d[0], d[1], d[2]), v3(d[3], d[4], d[5]), &dq, &dtv);
    o.q = qnormalize(qmul(s.q, dq));
    o.t = s.t + mul(qrot(s.q), dtv);
    o.vel = s.vel + v3(d[6], d[7], d[8]);
    o.ba = s.ba + v3(d[9], d[10], d[11]);
    o.bg = s.bg + v3(d[12], d[13], d[14]);
    store_state(v, b, gk, o);
#pragma unroll
    for (int a = 0; a < 15; a++) d[a] = 0.0;
    atomicMin(v.inc_k + w, k);
}
// the estimate theta (+) delta of the keyframes whose increment the back substitution touched, into the trial buffer (k_retract
// for the rest of the library); the last thing an incremental update does: inc_k is ready for the next one
__global__ void __launch_bounds__(256) k_inc_retract(View v) {
    const int w = blockIdx.y;
    const int lo = v.lo[w], hi = v.hi[w], from = v.inc_stop[w];
    const int k = (from & ~255) + (int)(blockIdx.x * 256 + threadIdx.x);
    if (blockIdx.x == 0 && threadIdx.x == 0) v.inc_k[w] = 0x7fffffff;
    if (k < lo || k < from || k >= hi) return;
    const long gk = (long)w * v.M + k;
    const int b = v.sel[w];
    const State s = load_state(v, b, gk);
    const double* d = v.delta + (size_t)gk * 15;
    State o;
    Q4 dq;
    V3 dtv;
    se3_exp(v3(d[0], d[1], d[2]), v3(d[3], d[4], d[5]), &dq, &dtv);
    o.q = qnormalize(qmul(s.q, dq));
    o.t = s.t + mul(qrot(s.q), dtv);
    o.vel = s.vel + v3(d[6], d[7], d[8]);
    o.ba = s.ba + v3(d[9], d[10], d[11]);
    o.bg = s.bg + v3(d[12], d[13], d[14]);
    store_state(v, b ^ 1, gk, o);
}
