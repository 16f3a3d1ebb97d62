// kernels/k2b_priors.inc -- K2b: the three priors, the marginal prior; K1 + K2 + K2b as one launch; the warm-start tail.
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ K2b
// delta of the marginal prior: [Local(xbar0 -> x_lo) (15); pose Local for lo+1 (6); lo+2 (6)]
VF_DI void marg_delta(const View& v, int w, int b, double (&d)[27]) {
    const int lo = v.lo[w];
    const double* xb = v.mp_x + (size_t)w * 48;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const long gk = (long)w * v.M + lo + j;
        const State s = load_state(v, b, gk);
        const Q4 qb = q4(xb[16 * j], xb[16 * j + 1], xb[16 * j + 2], xb[16 * j + 3]);
        const V3 tb = v3(xb[16 * j + 4], xb[16 * j + 5], xb[16 * j + 6]);
        const Xi6 xi = se3_log(qmul(qconj(qb), s.q), mulT(qrot(qb), s.t - tb));
        const int o = j == 0 ? 0 : 15 + 6 * (j - 1);
        d[o] = xi.w.x; d[o + 1] = xi.w.y; d[o + 2] = xi.w.z; d[o + 3] = xi.u.x; d[o + 4] = xi.u.y; d[o + 5] = xi.u.z;
        if (j == 0) {
            d[6] = s.vel.x - xb[7]; d[7] = s.vel.y - xb[8]; d[8] = s.vel.z - xb[9];
            d[9] = s.ba.x - xb[10]; d[10] = s.ba.y - xb[11]; d[11] = s.ba.z - xb[12];
            d[12] = s.bg.x - xb[13]; d[13] = s.bg.y - xb[14]; d[14] = s.bg.z - xb[15];
        }
    }
}

__global__ void __launch_bounds__(256) k_linearize_between(View v, int which) {
    linearize_between_factor<false>(v, which, (long)blockIdx.x * 256 + threadIdx.x);
}

__device__ __forceinline__ void linearize_prior_window(const View& v, int which, const int w) {
    if (w >= v.B || window_done(v, w)) return;
    if (v.relin_only && !v.relin[w]) return;
    if (v.inc_on && !v.inc_prior && v.inc_k[w] > v.lo[w] + 2) return;   // (the priors sit on the window's first three keyframes)
    const int b = v.sel[w] ^ which;
    if (v.mp_on[w] && v.hi[w] - v.lo[w] >= 3) {
        // marginal prior: gm = L d + eta, cost = 0.5 d^T L d + eta^T d (fixed linearisation point)
        double d[27];
        marg_delta(v, w, b, d);
        const double* L = v.mp_L + (size_t)w * 729;
        const double* eta = v.mp_eta + (size_t)w * 27;
        double* out = v.mp_out + ((size_t)b * v.B + w) * 28;
        double cost = 0.0;
        for (int i = 0; i < 27; i++) {
            double g = 0.0;
            for (int j = 0; j < 27; j++) g = fma(L[i * 27 + j], d[j], g);
            cost += d[i] * (0.5 * g + eta[i]);
            out[i] = g + eta[i];
        }
        out[27] = cost;
    }
    const int k = v.prior_k[w];
    if (k < v.lo[w] || k >= v.hi[w]) return;
    const long gk = (long)w * v.M + k;
    const double* in = v.prior_in + (size_t)w * PRIOR_IN;
    double* out = v.prior_out + ((size_t)b * v.B + w) * PRIOR_OUT;
    const State s = load_state(v, b, gk);
    const Q4 qp = q4(in[0], in[1], in[2], in[3]);
    const V3 tp = v3(in[4], in[5], in[6]);
    const M3 Rp = qrot(qp);
    const Xi6 xi = se3_log(qmul(qconj(qp), s.q), mulT(Rp, s.t - tp));
    M3 Jw, Q2;
    se3_jr_inv(xi, &Jw, &Q2);
    const double* sig = in + 16;
    const double r6[6] = {xi.w.x, xi.w.y, xi.w.z, xi.u.x, xi.u.y, xi.u.z};
    for (int i = 0; i < 225; i++) out[15 + i] = 0.0;
    for (int r = 0; r < 3; r++) {
        out[r] = r6[r] / sig[r];
        out[3 + r] = r6[3 + r] / sig[3 + r];
        for (int c = 0; c < 3; c++) {
            out[15 + r * 15 + c] = Jw.a[r * 3 + c] / sig[r];
            out[15 + (3 + r) * 15 + c] = Q2.a[r * 3 + c] / sig[3 + r];
            out[15 + (3 + r) * 15 + 3 + c] = Jw.a[r * 3 + c] / sig[3 + r];
        }
    }
    const double xs[9] = {s.vel.x, s.vel.y, s.vel.z, s.ba.x, s.ba.y, s.ba.z, s.bg.x, s.bg.y, s.bg.z};
    for (int i = 0; i < 9; i++) {
        out[6 + i] = (xs[i] - in[7 + i]) / sig[6 + i];
        out[15 + (6 + i) * 15 + 6 + i] = 1.0 / sig[6 + i];
    }
}
// K2 + K2b in one launch (large batches): the prior linearisations are one lane per window, i.e. a handful of waves
// running an 80 us latency chain; as the first workgroups of K2's grid they hide behind the between factors
__global__ void __launch_bounds__(256) k_linearize_between_prior(View v, int which, int nb_pri) {
    const int bx = blockIdx.x;
    if (bx < nb_pri) {      // one wave of windows per workgroup: four such chains on one CU ran 1.6 x longer
        if (threadIdx.x < 64) linearize_prior_window(v, which, bx * 64 + (int)threadIdx.x);
    } else linearize_between_factor<false>(v, which, (long)(bx - nb_pri) * 256 + threadIdx.x);
}
// K1 + K2 + K2b in ONE launch, for few windows (latency form): with a handful of windows each of the three kernels
// is a single latency chain (27 / 9 / 13 us), so running them side by side saves two of the three; for large
// batches they stay separate (K2 would inherit K1's register footprint here).
// (SH: the form time-sharded windows use, whatever the batch size)
template <bool SH>
__global__ void __launch_bounds__(K1_BLOCK, K1_WAVES) k_linearize_all(View v, int which, int nb_imu, int nb_btw) {
    const int bx = blockIdx.x;
    if (bx < nb_imu) linearize_imu_factor<SH>(v, which, (long)bx * K1_BLOCK + threadIdx.x);
    else if (bx < nb_imu + nb_btw) linearize_between_factor<SH>(v, which, (long)(bx - nb_imu) * K1_BLOCK + threadIdx.x);
    else linearize_prior_window(v, which, (bx - nb_imu - nb_btw) * K1_BLOCK + (int)threadIdx.x);
}

// ... and the three K2 launches of an engine that holds losses (View::btw_loss; linearize_between_factor<.., true>): kernels of
// their own, chosen on the host (launch.inc), so that the ones above stay what they were
__global__ void __launch_bounds__(256) k_linearize_between_robust(View v, int which) {
    linearize_between_factor<false, true>(v, which, (long)blockIdx.x * 256 + threadIdx.x);
}
__global__ void __launch_bounds__(256) k_linearize_between_prior_robust(View v, int which, int nb_pri) {
    const int bx = blockIdx.x;
    if (bx < nb_pri) {
        if (threadIdx.x < 64) linearize_prior_window(v, which, bx * 64 + (int)threadIdx.x);
    } else linearize_between_factor<false, true>(v, which, (long)(bx - nb_pri) * 256 + threadIdx.x);
}
__global__ void __launch_bounds__(K1_BLOCK, K1_WAVES) k_linearize_all_robust(View v, int which, int nb_imu, int nb_btw) {
    const int bx = blockIdx.x;
    if (bx < nb_imu) linearize_imu_factor<false>(v, which, (long)bx * K1_BLOCK + threadIdx.x);
    else if (bx < nb_imu + nb_btw) linearize_between_factor<false, true>(v, which, (long)(bx - nb_imu) * K1_BLOCK + threadIdx.x);
    else linearize_prior_window(v, which, (bx - nb_imu - nb_btw) * K1_BLOCK + (int)threadIdx.x);
}
// ... and of an engine that holds absolute factors (vf_engine_set_absolute; linearize_between_factor<.., true, true>, which reads the
// slots' kinds from btw_kind): kernels of their own again, so that the ones above stay what they were
__global__ void __launch_bounds__(256) k_linearize_between_abs(View v, int which, const int* btw_kind) {
    linearize_between_factor<false, true, true>(v, which, (long)blockIdx.x * 256 + threadIdx.x, btw_kind);
}
__global__ void __launch_bounds__(256) k_linearize_between_prior_abs(View v, int which, int nb_pri, const int* btw_kind) {
    const int bx = blockIdx.x;
    if (bx < nb_pri) {
        if (threadIdx.x < 64) linearize_prior_window(v, which, bx * 64 + (int)threadIdx.x);
    } else linearize_between_factor<false, true, true>(v, which, (long)(bx - nb_pri) * 256 + threadIdx.x, btw_kind);
}
__global__ void __launch_bounds__(K1_BLOCK, K1_WAVES) k_linearize_all_abs(View v, int which, int nb_imu, int nb_btw, const int* btw_kind) {
    const int bx = blockIdx.x;
    if (bx < nb_imu) linearize_imu_factor<false>(v, which, (long)bx * K1_BLOCK + threadIdx.x);
    else if (bx < nb_imu + nb_btw) linearize_between_factor<false, true, true>(v, which, (long)(bx - nb_imu) * K1_BLOCK + threadIdx.x, btw_kind);
    else linearize_prior_window(v, which, (bx - nb_imu - nb_btw) * K1_BLOCK + (int)threadIdx.x);
}

// Warm start of a fixed-lag update (vf_engine_slide directly after a solve): the linearisation of every factor that was
// in the window is still the one of the current states (an accepted trial's records became current with its states, a
// rejected one left both alone), so only the factors of the `nslid` appended keyframes and the priors (the marginal prior
// has just changed) are linearised.  H and g are then stale only at the two ends of a window whose last trial was
// rejected: fresh[w] = 1 + nslid tells k_assemble to redo just those tiles (fresh[w] = 1: all of them).
__global__ void __launch_bounds__(K1_BLOCK, K1_WAVES) k_linearize_tail(View v, int nslid) {
    const int bx = blockIdx.x, t = threadIdx.x;
    if (bx < v.B) {
        if (t < nslid) linearize_imu_factor<false>(v, 0, (long)bx * v.M + v.hi[bx] - 1 - t);
    } else if (bx < 2 * v.B) {
        const int w = bx - v.B;
        if (t < nslid) linearize_between_factor<false>(v, 0, (long)w * v.M + v.hi[w] - 1 - t);
    } else {
        const int w = (bx - 2 * v.B) * 64 + t;      // one wave of windows per workgroup
        if (t < 64) {
            if (w < v.B) v.fresh[w] = v.fresh[w] ? 1 : 1 + nslid;
            linearize_prior_window(v, 0, w);
        }
    }
}
__global__ void __launch_bounds__(K1_BLOCK, K1_WAVES) k_linearize_tail_robust(View v, int nslid) {
    const int bx = blockIdx.x, t = threadIdx.x;
    if (bx < v.B) {
        if (t < nslid) linearize_imu_factor<false>(v, 0, (long)bx * v.M + v.hi[bx] - 1 - t);
    } else if (bx < 2 * v.B) {
        const int w = bx - v.B;
        if (t < nslid) linearize_between_factor<false, true>(v, 0, (long)w * v.M + v.hi[w] - 1 - t);
    } else {
        const int w = (bx - 2 * v.B) * 64 + t;
        if (t < 64) {
            if (w < v.B) v.fresh[w] = v.fresh[w] ? 1 : 1 + nslid;
            linearize_prior_window(v, 0, w);
        }
    }
}
__global__ void __launch_bounds__(K1_BLOCK, K1_WAVES) k_linearize_tail_abs(View v, int nslid, const int* btw_kind) {
    const int bx = blockIdx.x, t = threadIdx.x;
    if (bx < v.B) {
        if (t < nslid) linearize_imu_factor<false>(v, 0, (long)bx * v.M + v.hi[bx] - 1 - t);
    } else if (bx < 2 * v.B) {
        const int w = bx - v.B;
        if (t < nslid) linearize_between_factor<false, true, true>(v, 0, (long)w * v.M + v.hi[w] - 1 - t, btw_kind);
    } else {
        const int w = (bx - 2 * v.B) * 64 + t;
        if (t < 64) {
            if (w < v.B) v.fresh[w] = v.fresh[w] ? 1 : 1 + nslid;
            linearize_prior_window(v, 0, w);
        }
    }
}
