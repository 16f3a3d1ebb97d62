// kernels/far.inc -- far between factors: linearisation, gradient, Woodbury columns and the small dense combine.
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ---- "far" between factors (View::x_*): BetweenFactor<Pose3> on ANY pair of keyframes of a window -- a span wider than
// the band, or a second factor on an end key (loop closures; GraphManager.cpp:83-88 takes any pair of keys).  They stay
// out of the banded H: the solve treats them as a low-rank correction (launch_extra_* below, vf_engine_solve).
// A window's slots: first its LINEAR far factors (View::xl_*: far factors whose older keyframe has been marginalised), then
// the entries of x_a / x_b.  FarRef resolves a slot: kind -1 = empty or reaching outside the window (no cost, no rows).
VF_DI void marg_delta(const View& v, int w, int b, double (&d)[27]);
#include "../vf_far.hpp"
// One lane per (window, index): entry `index` of the window's nonlinear list, and far end `index` of its linear far factor
// (the six rows that belong to it).
// RB: the engine holds losses of far factors (View::x_loss; far_loss).  An entry the loss changes -- not LOSS_NONE, not a Huber inlier,
// not s = 0 -- is rewritten in its square-root form by the second pass K2 applies to a band factor (robustify_between, over the 78
// words the lane has just stored); every consumer of x_out reads r^ and J^ and knows nothing of losses.  The RB = false instance
// reads no new word: the kernel as it was before far factors took losses, chosen on the host (launch.inc).  The linear far factor
// (xl_*) has no loss: a robust far factor enters it at the weight of the linearisation it is marginalised at.
template <bool RB>
__global__ void __launch_bounds__(64) k_linearize_extra(View v, int which) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= v.B * v.x_max) return;
    const int w = i / v.x_max, s = i - w * v.x_max;
    if (window_done(v, w)) return;
    const int b = v.sel[w] ^ which, lo = v.lo[w], hi = v.hi[w];
    {
        const int a = v.x_a[i], kb = v.x_b[i];
        double* out = v.x_out + ((size_t)b * v.B * v.x_max + i) * BTW_OUT;
        if (a < lo || kb >= hi || a >= kb) { for (int f = 0; f < BTW_OUT; f++) out[f] = 0.0; }
        else {
            between_core<false>(v, b, (long)w * v.M + a, (long)w * v.M + kb, v.x_in + (size_t)i * BTW_IN, 1, out, 1, true);
            if constexpr (RB) {
                const FarLoss fl = far_loss(v, i);
                if (fl.loss != LOSS_NONE) robustify_between<1>(out, fl.loss, fl.k);
            }
        }
    }
    double* lout = v.xl_out + ((size_t)b * v.B + w) * 6 * v.x_max + 6 * s;
    const int nl = v.xl_n[w];
    if (s < nl && hi - lo > 3 && v.mp_on[w]) {
        double dh[27];
        marg_delta(v, w, b, dh);
        const double* U = v.xl_U + ((size_t)w * 6 * v.x_max + 6 * s) * xl_ld(v);
        double acc[6];
        for (int j = 0; j < 6; j++) {
            acc[j] = v.xl_r0[(size_t)w * 6 * v.x_max + 6 * s + j];
            for (int c = 0; c < 27; c++) acc[j] = fma(U[j * xl_ld(v) + c], dh[c], acc[j]);
        }
        for (int e = 0; e < nl; e++) {
            const double* xb = v.xl_bx + ((size_t)w * v.x_max + e) * 7;
            const State st = load_state(v, b, (long)w * v.M + v.xl_b[w * v.x_max + e]);
            const Q4 qb = q4(xb[0], xb[1], xb[2], xb[3]);
            const Xi6 xi = se3_log(qmul(qconj(qb), st.q), mulT(qrot(qb), st.t - v3(xb[4], xb[5], xb[6])));
            const double d6[6] = {xi.w.x, xi.w.y, xi.w.z, xi.u.x, xi.u.y, xi.u.z};
            for (int j = 0; j < 6; j++)
                for (int c = 0; c < 6; c++) acc[j] = fma(U[j * xl_ld(v) + 27 + 6 * e + c], d6[c], acc[j]);
        }
        for (int j = 0; j < 6; j++) lout[j] = acc[j];
    } else
        for (int j = 0; j < 6; j++) lout[j] = 0.0;
}
// g += J^T r of the far factors, for the windows whose rows K3 has just rewritten (same test as k_assemble; engines that
// hold far factors never warm-start, so "rewritten" means the whole window)
__global__ void __launch_bounds__(64) k_extra_gradient(View v) {
    const int w = blockIdx.x, lane = threadIdx.x;
    if (!v.fresh[w] || window_done(v, w)) return;
    const int b = v.sel[w];
    __shared__ int kb_l[MAX_EXTRA_BIG];
    far_ends(v, w, lane, kb_l);
    for (int s = 0; s < v.x_max; s++) {              // sequential over the slots: two factors may share a keyframe
        const FarRef f = far_ref(v, w, s);
        far_jt_apply(v, w, f, b, lane, kb_l, [&](int r) { return far_res(v, w, f, b, r); }, v.gvec);
    }
}
// right-hand side number (s, j) of the low-rank correction: row j of the far factor in slot s of every window, scattered
// over the keyframes it touches, into a zeroed increment-shaped buffer
__global__ void __launch_bounds__(64) k_extra_rhs(View v, int s, int j, double* __restrict__ gtmp) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= v.B || window_done(v, w)) return;
    far_scatter<false>(v, w, far_ref(v, w, s), v.sel[w], j, gtmp + (size_t)w * v.M * 15, 1);
}
// ---- the Woodbury columns of a SINGLE-window engine as one batch (vf_engine.hip "far_columns"): window q of the view `c` (an
// engine of 6 x MAX_EXTRA windows with the same capacity) is a copy of the window's block rows of H with column q of U as its
// right-hand side, so that ONE partitioned solve of `c` returns every column of Z where the window's own solver would be run
// once per column.  Same kernels on the same numbers: the same bits.
__global__ void __launch_bounds__(256) k_cols_prepare(View v, View c, int ncols) {
    const int k = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int lo = v.lo[0], hi = v.hi[0];
    if (window_done(v, 0)) ncols = 0;            // (the termination rule has finished the window: its column windows are empty too)
    // (every window of `c` takes part in the launch -- the separator arrays are laid out by its window count -- the ones beyond
    // the columns in use as empty windows)
    // (mp_on: the solver asks it whether row lo + 2 carries the marginal prior's coupling to lo, the block at H_DX)
    if (k == 0 && tid == 0) { c.lo[q] = q < ncols ? lo : 0; c.hi[q] = q < ncols ? hi : 0; c.lambda[q] = v.lambda[0]; c.fail[q] = 0; c.mp_on[q] = v.mp_on[0]; }
    if (k < lo || k >= hi || q >= ncols) return;
    const double* __restrict__ src = v.H + (size_t)k * HROW;
    double* __restrict__ dst = c.H + ((size_t)q * c.M + k) * HROW;
    for (int i = tid; i < HROW; i += 256) dst[i] = src[i];
    if (tid < 15) c.gvec[((size_t)q * c.M + k) * 15 + tid] = 0.0;
}
__global__ void __launch_bounds__(64) k_cols_rhs(View v, View c, int ncols) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= ncols || window_done(v, 0)) return;
    far_scatter<false>(v, 0, far_ref(v, 0, q / 6), v.sel[0], q % 6, c.gvec + (size_t)q * c.M * 15, 1);
}
__global__ void __launch_bounds__(64) k_cols_fail(View v, View c, int ncols) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q < ncols && !window_done(v, 0) && c.fail[q]) v.fail[0] = 1;
}
void launch_cols_prepare(const View& v, const View& c, int ncols, hipStream_t s) {
    hipLaunchKernelGGL(k_cols_prepare, dim3((unsigned)v.M, (unsigned)c.B), dim3(256), 0, s, v, c, ncols);
    hipLaunchKernelGGL(k_cols_rhs, dim3((unsigned)((ncols + 63) / 64)), dim3(64), 0, s, v, c, ncols);
}
void launch_cols_fail(const View& v, const View& c, int ncols, hipStream_t s) {
    hipLaunchKernelGGL(k_cols_fail, dim3((unsigned)((ncols + 63) / 64)), dim3(64), 0, s, v, c, ncols);
}
// delta = y - Z (I + U^T Z)^-1 U^T y  (Woodbury; A = H_band + lambda I, y = -A^-1 g in v.delta, column q of Zm = -A^-1 u_q as
// the band solver returned it for the right-hand side u_q): one workgroup per window, the m = 6 x_max square system in LDS.
// BIG (engines made with max_far_factors > VF_MAX_EXTRA; m up to 6 MAX_EXTRA_BIG = 192): the system lives in the window's
// View::far_scratch and the three steps are three launches -- k_extra_fill (a workgroup per slot), this kernel (the elimination),
// k_extra_apply (a workgroup per 256 entries of delta); every entry is formed by the same chain of fma in the same order as in the
// LDS form, so a window with eight or fewer far factors gets the same bits from either.
constexpr int BIG_LD = 6 * MAX_EXTRA_BIG + 1;
constexpr size_t SMALL_SCRATCH = 64;     // doubles of far_scratch per window on engines made for <= MAX_EXTRA far factors (the solution: 6 MAX_EXTRA)
constexpr size_t BIG_CVEC = (size_t)6 * MAX_EXTRA_BIG * BIG_LD;     // offset of the solution (6 MAX_EXTRA_BIG doubles) in far_scratch
static_assert(BIG_CVEC + 6 * MAX_EXTRA_BIG <= FAR_SCRATCH, "far_scratch holds the Woodbury system and its solution");
__global__ void __launch_bounds__(256) k_extra_fill(View v, const double* __restrict__ Zm, size_t zstride, int slots) {
    __shared__ double J[6 * FAR_NCMAX];
    __shared__ int off[FAR_NCMAX];
    const int s = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
    if (v.hi[w] - v.lo[w] <= 0 || window_done(v, w)) return;
    double* const C = v.far_scratch + (size_t)w * FAR_SCRATCH;
    const int m = 6 * slots, b = v.sel[w];
    const int nc = far_stage<false>(v, w, far_ref(v, w, s), b, tid, 256, J, off);
    __syncthreads();
    for (int e = tid; e < 6 * (m + 1); e += 256) {
        const int j = e / (m + 1), q = e - j * (m + 1), p = 6 * s + j;
        const double* col = (q < m ? Zm + (size_t)q * zstride : v.delta) + (size_t)w * v.M * 15;
        double acc = 0.0;
        for (int c = 0; c < nc; c++) acc = fma(J[j * FAR_NCMAX + c], col[off[c]], acc);
        C[p * BIG_LD + q] = q < m ? (p == q ? 1.0 : 0.0) - acc : acc;
    }
}
// (both forms: the solution of the small system is in the window's far_scratch -- at BIG_CVEC of FAR_SCRATCH doubles, or the
// first of SMALL_SCRATCH)
template <bool BIG>
__global__ void __launch_bounds__(256) k_extra_apply(View v, const double* __restrict__ Zm, size_t zstride, int slots) {
    const int w = blockIdx.y;
    if (v.hi[w] - v.lo[w] <= 0 || window_done(v, w)) return;
    const int m = 6 * slots, lo = v.lo[w], hi = v.hi[w], e = blockIdx.x * 256 + threadIdx.x;
    __shared__ double cvec[6 * MAX_EXTRA_BIG];
    if ((int)threadIdx.x < m) cvec[threadIdx.x] = v.far_scratch[BIG ? (size_t)w * FAR_SCRATCH + BIG_CVEC + threadIdx.x : (size_t)w * SMALL_SCRATCH + threadIdx.x];
    __syncthreads();
    if (e >= (hi - lo) * 15) return;
    const size_t o = ((size_t)w * v.M + lo) * 15 + e;
    double acc = v.delta[o];
    for (int q = 0; q < m; q++) acc = fma(cvec[q], Zm[(size_t)q * zstride + o], acc);
    v.delta[o] = acc;
}
template <bool BIG>
__global__ void __launch_bounds__(BIG ? 1024 : 256) k_extra_combine(View v, const double* __restrict__ Zm, size_t zstride, int slots) {
    constexpr int MM = 6 * (BIG ? MAX_EXTRA_BIG : MAX_EXTRA), LD = MM + 1, NT = BIG ? 1024 : 256;
    __shared__ double C_lds[BIG ? 1 : MM * LD];
    __shared__ double cvec[MM];
    double* const C = BIG ? v.far_scratch + (size_t)blockIdx.x * FAR_SCRATCH : C_lds;
    const int w = blockIdx.x, tid = threadIdx.x;
    if (v.hi[w] - v.lo[w] <= 0 || window_done(v, w)) return;
    const int m = 6 * slots, b = v.sel[w];      // slots in use (the rest are empty in every window)
    // C[p][q] = delta_pq - u_p . Zm_q  (= delta_pq + u_p^T A^-1 u_q), C[p][m] = u_p . y
    if constexpr (!BIG) {
        for (int e = tid; e < m * (m + 1); e += NT) {
            const int p = e / (m + 1), q = e - p * (m + 1);
            const int s = p / 6, j = p - 6 * s;
            const FarRef f = far_ref(v, w, s);
            double acc = 0.0;
            if (f.kind >= 0) {
                const double* col = (q < m ? Zm + (size_t)q * zstride : v.delta) + (size_t)w * v.M * 15;
                const int nc = far_cols(f);
                for (int c = 0; c < nc; c++) {
                    int k, d;
                    far_col(v, w, f, c, k, d);
                    acc = fma(far_jac(v, w, f, b, j, c), col[(size_t)k * 15 + d], acc);
                }
            }
            C[p * LD + q] = q < m ? (p == q ? 1.0 : 0.0) - acc : acc;
        }
        __syncthreads();
    }
    // Gaussian elimination (C is symmetric positive definite: I + U^T A^-1 U), entry-parallel
    if constexpr (BIG) {
        // The same elimination, NB pivots at a time: the pivots' columns (from the first of them down) and rows (from it to the right)
        // are eliminated among themselves in LDS, then every entry below and to the right takes its NB updates in one visit to device
        // memory instead of NB -- the updates an entry receives, their operands and their order (pivot after pivot, as
        // fma(-C[p][c] inv_c, C[c][q], .)) are those of the loop below.
        constexpr int NB = 8;
        __shared__ double Lp[MM * NB], Up[NB * LD], invs[NB];
        for (int c0 = 0; c0 < m; c0 += NB) {
            const int nb = min(NB, m - c0), rows = m - c0, cols = m + 1 - c0;
            __syncthreads();
            for (int e = tid; e < rows * nb; e += NT) { const int p = e / nb, j = e - p * nb; Lp[p * NB + j] = C[(c0 + p) * LD + c0 + j]; }
            for (int e = tid; e < nb * cols; e += NT) { const int i = e / cols, q = e - i * cols; Up[i * LD + q] = C[(c0 + i) * LD + c0 + q]; }
            __syncthreads();
            for (int j = 0; j < nb; j++) {
                const double inv = 1.0 / Up[j * LD + j];
                if (tid == 0) invs[j] = inv;
                __syncthreads();
                // (the pivot block is in both arrays: both copies take the same updates from the same operands)
                const int np = (rows - 1 - j) * (nb - 1 - j), nu = (nb - 1 - j) * (cols - 1 - j);
                for (int e = tid; e < np + nu; e += NT) {
                    if (e < np) {
                        const int p = j + 1 + e / (nb - 1 - j), j2 = j + 1 + (e - (e / (nb - 1 - j)) * (nb - 1 - j));
                        Lp[p * NB + j2] = fma(-Lp[p * NB + j] * inv, Up[j * LD + j2], Lp[p * NB + j2]);
                    } else {
                        const int x = e - np, i = j + 1 + x / (cols - 1 - j), q = j + 1 + (x - (x / (cols - 1 - j)) * (cols - 1 - j));
                        Up[i * LD + q] = fma(-Lp[i * NB + j] * inv, Up[j * LD + q], Up[i * LD + q]);
                    }
                }
                __syncthreads();
            }
            // the pivots' rows are final: back where the back substitution reads them
            for (int e = tid; e < nb * cols; e += NT) { const int i = e / cols, q = e - i * cols; C[(c0 + i) * LD + c0 + q] = Up[i * LD + q]; }
            const int tr = rows - nb, tc = cols - nb;                    // the entries below and to the right
            for (int e0 = 0; e0 < tr * tc; e0 += 4 * NT) {
                double x[4];
                int pp[4], qq[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int e = e0 + u * NT + tid;
                    pp[u] = e < tr * tc ? nb + e / tc : -1;
                    qq[u] = e < tr * tc ? nb + (e - (e / tc) * tc) : 0;
                    x[u] = pp[u] >= 0 ? C[(c0 + pp[u]) * LD + c0 + qq[u]] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (pp[u] < 0) continue;
                    for (int j = 0; j < nb; j++) x[u] = fma(-Lp[pp[u] * NB + j] * invs[j], Up[j * LD + qq[u]], x[u]);
                    C[(c0 + pp[u]) * LD + c0 + qq[u]] = x[u];
                }
            }
        }
        __syncthreads();
    } else {
        for (int c = 0; c < m; c++) {
            const double inv = 1.0 / C[c * LD + c];
            __syncthreads();
            const int rem = m - 1 - c;
            for (int e = tid; e < rem * (rem + 1); e += NT) {
                const int p = c + 1 + e / (rem + 1), q = c + 1 + (e - (e / (rem + 1)) * (rem + 1));
                C[p * LD + q] = fma(-C[p * LD + c] * inv, C[c * LD + q], C[p * LD + q]);
            }
            __syncthreads();
        }
    }
    if constexpr (BIG) {
        // (the rows come out of device memory through LDS, fetched by the whole workgroup; the chain of fma is one thread's, as below)
        __shared__ double rowbuf[MM + 1];
        for (int p = m - 1; p >= 0; p--) {
            for (int q = p + tid; q <= m; q += NT) rowbuf[q] = C[p * LD + q];
            __syncthreads();
            if (tid == 0) {
                double t = rowbuf[m];
                for (int q = p + 1; q < m; q++) t = fma(-rowbuf[q], cvec[q], t);
                cvec[p] = t / rowbuf[p];
            }
            __syncthreads();
        }
    } else if (tid == 0) {
        for (int p = m - 1; p >= 0; p--) {
            double t = C[p * LD + m];
            for (int q = p + 1; q < m; q++) t = fma(-C[p * LD + q], cvec[q], t);
            cvec[p] = t / C[p * LD + p];
        }
    }
    __syncthreads();
    // delta = y + sum_q c_q Zm_q over the window's keyframes: k_extra_apply, on as many workgroups as the window has entries / 256
    if (tid < m) {
        if constexpr (BIG) C[BIG_CVEC + tid] = cvec[tid];
        else v.far_scratch[(size_t)w * SMALL_SCRATCH + tid] = cvec[tid];
    }
}
