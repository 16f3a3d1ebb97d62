// kernels/k4_selinv_far.inc -- K4s with far factors alive: the low-rank downdate of the band's marginal covariances.
// A section of vf_kernels.hip (ONE translation unit); included from there after k4_selinv.inc, inside namespace vf, never
// compiled by itself.
//
// The band solver holds A = H_band; the far factors (far.inc) add U U^T, U the whitened far rows (m = 6 x slots in use columns).
// With Z = A^-1 U, C = I + U^T Z = R R^T and Y = Z R^-T, the covariance of H = A + U U^T is
//     Sigma = A^-1 - Y Y^T,    so    Sigma_kk -= Y_k Y_k^T,   Sigma_{k+1,k} -= Y_{k+1} Y_k^T
// (Y_k: the 15 rows of keyframe k), applied to what k_band_selinv left in sig.  Five kernels per group of windows:
//   k_farcov_rhs       U scattered into the zeroed Z
//   k_farcov_forward   Z = A^-1 U on the panels of the undamped sweep: forward substitution (one lane per column)
//   k_farcov_back      ... and back substitution
//   k_farcov_chol<BIG> C and its Cholesky factor R (in LDS for m <= 6 MAX_EXTRA, in device memory beyond or with far_big)
//   k_farcov_downdate  Y of keyframes k and k + 1, then the two blocks of slot k
// Windows without a live slot, and windows whose sweep (or C) was not positive definite, are left alone: their Sigma keeps the
// bits k_band_selinv gave it.
VF_DI bool far_live(const View& v, int w, int slots) {
    for (int s = 0; s < slots; s++)
        if (far_ref(v, w, s).kind >= 0) return true;
    return false;
}
VF_DI bool farcov_skip(const View& v, const FarCov& fc, int w) {
    const int lo = v.lo[w], hi = v.hi[w];
    return hi - lo <= 0 || hi > v.M || lo < 0 || fc.failed[w] || !far_live(v, w, fc.slots);
}
// column q of U (row q % 6 of slot q / 6) scattered over the keyframes it touches into the zeroed window, a lane per column: columns
// that land on the same (keyframe, dof) add up, as in k_extra_rhs / k_cols_rhs
__global__ void __launch_bounds__(256) k_farcov_rhs(View v, FarCov fc) {
    const int w = fc.w0 + blockIdx.x, q = threadIdx.x, m = fc.m;
    if (q >= m || farcov_skip(v, fc, w)) return;
    const int lo = v.lo[w], hi = v.hi[w];
    double* __restrict__ Z = fc.Z + (size_t)blockIdx.x * fc.zwin;
    for (int i = lo * 15; i < hi * 15; i++) Z[(size_t)i * m + q] = 0.0;
    far_scatter<true>(v, w, far_ref(v, w, q / 6), v.sel[w], q % 6, Z + q, (size_t)m);
}
// Z = A^-1 U on the panels of the undamped sweep, as two launches of one wave per (window, 64 columns), a lane per column:
//   k_farcov_forward  y_k = L_kk^-1 (u_k - the B updates of k-1 .. k-3) = U_k^T r_k, then the updates of S_k: B_k y_k
//   k_farcov_back     x_k = U_k (y_k - B_k^T x_S)
// with S_k = [k+1: 15][k+2: pose][k+3: pose], B_k and U_k read from the panel exactly as k_band_selinv reads them (rows of keyframes
// at or beyond hi zeroed), the next panel fetched into registers while the current step computes and staged in LDS (forward: B as
// it is and U transposed; back: B transposed and U -- every product reads one contiguous row, broadcast to the wave).  The lane's
// pending updates (forward) and its last solved keyframes (back), 27 doubles each, live in LDS, a column per lane, so that the
// 27-row products are loops instead of fully unrolled chains.  y overwrites u in
// Z, x overwrites y.  (Offsets within a keyframe's rows are 32-bit: 30 m doubles at most.)
constexpr int FC_PF = (SI_ENT + 63) / 64;       // panel entries per lane
constexpr int FC_BT = 28;                        // row stride of B^T in LDS
static_assert(15 * FC_BT <= 27 * SI_LD, "B^T fits where B goes");
struct FarPanel {
    double PB[27 * SI_LD], PU[15 * SI_LD];
};
VF_DI void farcov_fetch(const View& v, int w, int k, int hi, int lane, double (&pf)[FC_PF]) {
    const double* __restrict__ p = v.Lp + ((size_t)w * v.M + k) * PANEL;
#pragma unroll
    for (int t = 0; t < FC_PF; t++) {
        const int e = lane + 64 * t, r = e / 15, c = e - 15 * (e / 15);
        double x = 0.0;
        if (e < SI_ENT && (r >= 27 || k + 1 + (r < 15 ? 0 : (r < 21 ? 1 : 2)) < hi)) x = p[panel_idx(r < 27 ? r : r + 1, c)];
        pf[t] = x;
    }
}
template <bool BACK>
VF_DI void farcov_stage(FarPanel& P, int lane, const double (&pf)[FC_PF]) {
#pragma unroll
    for (int t = 0; t < FC_PF; t++) {
        const int e = lane + 64 * t, r = e / 15, c = e - 15 * (e / 15);
        if (e < SI_ENT) {
            if (r < 27) { if (BACK) P.PB[c * FC_BT + r] = pf[t]; else P.PB[r * SI_LD + c] = pf[t]; }
            else { if (BACK) P.PU[(r - 27) * SI_LD + c] = pf[t]; else P.PU[c * SI_LD + r - 27] = pf[t]; }
        }
    }
}
__global__ void __launch_bounds__(64) k_farcov_forward(View v, FarCov fc) {
    const int w = fc.w0 + blockIdx.x, lane = threadIdx.x, col = blockIdx.y * 64 + lane, m = fc.m;
    if (farcov_skip(v, fc, w)) return;
    const int lo = v.lo[w], hi = v.hi[w];
    const bool mine = col < m;
    double* __restrict__ zc = fc.Z + (size_t)blockIdx.x * fc.zwin + (mine ? col : 0);
    __shared__ FarPanel P;
    __shared__ double PS[27 * 64];       // the lane's pending updates of [k: 15][k+1: pose][k+2: pose], entry i at PS[64 i + lane]
    for (int i = 0; i < 27; i++) PS[64 * i + lane] = 0.0;
    double pf[FC_PF], nx[15];
    farcov_fetch(v, w, lo, hi, lane, pf);
#pragma unroll
    for (int d = 0; d < 15; d++) nx[d] = mine ? zc[((size_t)lo * 15 + d) * m] : 0.0;
#pragma unroll 1
    for (int k = lo; k < hi; k++) {
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
        if (k + 1 < hi && mine)          // (behind the stores, as in k_farcov_back)
#pragma unroll
            for (int d = 0; d < 15; d++) nx[d] = zk[(15 + d) * m];
        // pending of k + 1 = [k+1: 15][k+2: pose][k+3: pose]: the old pose rows of k+1 / k+2 (rows 15.. / 21..) plus B_k y, row by
        // row in an order that reads every old row before it is overwritten (each lane its own column)
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
__global__ void __launch_bounds__(64) k_farcov_back(View v, FarCov fc) {
    const int w = fc.w0 + blockIdx.x, lane = threadIdx.x, col = blockIdx.y * 64 + lane, m = fc.m;
    if (farcov_skip(v, fc, w)) return;
    const int lo = v.lo[w], hi = v.hi[w];
    const bool mine = col < m;
    double* __restrict__ zc = fc.Z + (size_t)blockIdx.x * fc.zwin + (mine ? col : 0);
    __shared__ FarPanel P;
    __shared__ double XS[27 * 64];       // the lane's x_S: [k+1: 15][k+2: pose][k+3: pose], entry i at XS[64 i + lane]
    for (int i = 0; i < 27; i++) XS[64 * i + lane] = 0.0;
    double pf[FC_PF], nx[15];
    farcov_fetch(v, w, hi - 1, hi, lane, pf);
#pragma unroll
    for (int d = 0; d < 15; d++) nx[d] = mine ? zc[((size_t)(hi - 1) * 15 + d) * m] : 0.0;
#pragma unroll 1
    for (int k = hi - 1; k >= lo; k--) {
        farcov_stage<true>(P, lane, pf);
        __syncthreads();
        if (k > lo) farcov_fetch(v, w, k - 1, hi, lane, pf);
        double t[15];
#pragma unroll
        for (int j = 0; j < 15; j++) {
            double s = nx[j];
#pragma unroll 9
            for (int i = 0; i < 27; i++) s = fma(-P.PB[j * FC_BT + i], XS[64 * i + lane], s);
            t[j] = s;
        }
        double* __restrict__ zk = zc + (size_t)k * 15 * m;
        // x_S of k - 1 = [k: 15][k+1: pose][k+2: pose]: the pose rows of k+1 move down first (each lane its own column)
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
        if (k > lo && mine)
#pragma unroll
            for (int d = 0; d < 15; d++) nx[d] = zk[(d - 15) * m];
        __syncthreads();
    }
}
// C[p][q] = delta_pq + u_p . z_q (lower triangle; u_p through far_col offsets as k_extra_combine forms it, slot by slot with the
// slot's six rows staged in LDS), then C = R R^T by right-looking Cholesky, entry-parallel.  BIG: C in the window's part of
// FarCov::C throughout; else in LDS, R copied there at the end.  Every entry takes the same chain of operations in both forms,
// so they give the same bits.
template <bool BIG>
__global__ void __launch_bounds__(256) k_farcov_chol(View v, FarCov fc) {
    constexpr int MM = 6 * MAX_EXTRA, NT = 256;
    __shared__ double C_lds[BIG ? 1 : MM * MM];
    __shared__ double J[6 * FAR_NCMAX];
    __shared__ int off[FAR_NCMAX];
    const int w = fc.w0 + blockIdx.x, tid = threadIdx.x, m = fc.m;
    if (farcov_skip(v, fc, w)) return;
    const int b = v.sel[w];
    const double* __restrict__ Z = fc.Z + (size_t)blockIdx.x * fc.zwin;
    double* const Rg = fc.C + (size_t)blockIdx.x * fc.cwin;
    double* const C = BIG ? Rg : C_lds;
    for (int s = 0; s < fc.slots; s++) {
        __syncthreads();
        const int nc = far_stage<true>(v, w, far_ref(v, w, s), b, tid, NT, J, off);
        __syncthreads();
        for (int q = tid; q < 6 * s + 6; q += NT) {
            double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < nc; c++) {
                const double z = off[c] >= 0 ? Z[(size_t)off[c] * m + q] : 0.0;
#pragma unroll
                for (int j = 0; j < 6; j++) acc[j] = fma(J[j * FAR_NCMAX + c], z, acc[j]);
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const int p = 6 * s + j;
                if (p >= q) C[p * m + q] = (p == q ? 1.0 : 0.0) + acc[j];
            }
        }
    }
    for (int c = 0; c < m; c++) {
        __syncthreads();
        const double dg = C[c * m + c];
        if (!(dg > 0.0) || !(dg < INFINITY)) {        // (the same value in every thread: the whole workgroup leaves)
            if (tid == 0) fc.failed[w] = 1;
            return;
        }
        const double rd = sqrt(dg);
        __syncthreads();
        for (int p = c + tid; p < m; p += NT) C[p * m + c] = p == c ? rd : C[p * m + c] / rd;
        __syncthreads();
        const int rem = m - 1 - c;
        for (int e = tid; e < rem * rem; e += NT) {
            const int p = c + 1 + e / rem, q = c + 1 + (e - (e / rem) * rem);
            if (p >= q) C[p * m + q] = fma(-C[p * m + c], C[q * m + c], C[p * m + q]);
        }
    }
    if constexpr (!BIG) {
        __syncthreads();
        for (int e = tid; e < m * m; e += NT) {
            const int p = e / m, q = e - (e / m) * m;
            if (p >= q) Rg[e] = C[e];
        }
    }
}
// One workgroup per (keyframe slot k, window): the 30 rows of Y_k and Y_{k+1} (Y_{k+1} = 0 for the window's last keyframe) --
// rows of Z are contiguous per keyframe, read at once into LDS and solved there in place, a thread per row
// (y_p = (z_p - sum_{q < p} R_pq y_q) / R_pp: rows are independent, the same chain in both workgroups that need a row) -- then
// the 120 + 225 entries of the two blocks, a thread per entry over the m columns (VALU, operands from LDS).
constexpr int FC_YROWS = 30;
__global__ void __launch_bounds__(64) k_farcov_downdate(View v, FarCov fc, double* __restrict__ sig) {
    extern __shared__ double ylds[];                  // [30][m + 1]
    const int w = fc.w0 + blockIdx.y, tid = threadIdx.x, m = fc.m, ld = m + 1;
    if (farcov_skip(v, fc, w)) return;
    const int k = v.lo[w] + blockIdx.x, hi = v.hi[w];
    if (k >= hi) return;
    const double* __restrict__ Z = fc.Z + (size_t)blockIdx.y * fc.zwin + (size_t)k * 15 * m;
    const double* __restrict__ R = fc.C + (size_t)blockIdx.y * fc.cwin;
    const int rows = k + 1 < hi ? FC_YROWS : 15;
    for (int e = tid; e < FC_YROWS * m; e += 64) {
        const int i = e / m, q = e - (e / m) * m;
        ylds[i * ld + q] = i < rows ? Z[e] : 0.0;
    }
    __syncthreads();
    if (tid < rows) {
        double* __restrict__ y = ylds + tid * ld;
        for (int p = 0; p < m; p++) {
            double s = y[p];
            for (int q = 0; q < p; q++) s = fma(-R[p * m + q], y[q], s);
            y[p] = s / R[p * m + p];
        }
    }
    __syncthreads();
    double* __restrict__ out = sig + ((size_t)w * v.M + k) * SIG_SLOT;
    for (int e = tid; e < SIG_SLOT; e += 64) {
        int a, c;
        if (e < 120) {
            a = 0;
            while ((a + 1) * (a + 2) / 2 <= e) a++;
            c = e - a * (a + 1) / 2;
        } else {
            a = 15 + (e - 120) / 15;
            c = (e - 120) % 15;
        }
        const double* __restrict__ ya = ylds + a * ld;
        const double* __restrict__ yc = ylds + c * ld;
        double s = 0.0;
        for (int q = 0; q < m; q++) s = fma(ya[q], yc[q], s);
        out[e] -= s;
    }
}
// Z = A^-1 U and R of the windows' far systems, without the downdate of sig (the loop-closure gate, kclosure.inc, reads Z and R itself)
void launch_farcov_system(const View& v, const FarCov& fc, int nw, hipStream_t s) {
    const unsigned cb = (unsigned)((fc.m + 63) / 64);
    hipLaunchKernelGGL(k_farcov_rhs, dim3((unsigned)nw), dim3(64 * cb), 0, s, v, fc);
    hipLaunchKernelGGL(k_farcov_forward, dim3((unsigned)nw, cb), dim3(64), 0, s, v, fc);
    hipLaunchKernelGGL(k_farcov_back, dim3((unsigned)nw, cb), dim3(64), 0, s, v, fc);
    if (far_big_form(v, fc.slots)) hipLaunchKernelGGL(k_farcov_chol<true>, dim3((unsigned)nw), dim3(256), 0, s, v, fc);
    else hipLaunchKernelGGL(k_farcov_chol<false>, dim3((unsigned)nw), dim3(256), 0, s, v, fc);
}
void launch_farcov(const View& v, const FarCov& fc, int nw, double* sig, hipStream_t s) {
    launch_farcov_system(v, fc, nw, s);
    hipLaunchKernelGGL(k_farcov_downdate, dim3((unsigned)v.M, (unsigned)nw), dim3(64), (size_t)FC_YROWS * (fc.m + 1) * sizeof(double), s,
                       v, fc, sig);
}
