// kernels/k4_selinv.inc -- K4s: marginal covariances of a window's keyframes from the Cholesky panels of an undamped forward
// sweep (selected inversion, the block form of Takahashi's recursion).
// A section of vf_kernels.hip (ONE translation unit); included from there, inside namespace vf, never compiled by itself.
//
// One wave per window, backward from hi - 1 to lo.  With S_k = [k+1: 15][k+2: pose][k+3: pose] (27 rows), B_k = L[S_k, k] and
// U_k = L_kk^-T (both from the panel of k) and the 27 x 27 block Sigma_SS of S_k (zero at k = hi - 1):
//     X_k        = B_k U_k^T                          (27 x 15)
//     Sigma_Sk   = -Sigma_SS X_k                      (27 x 15)
//     Sigma_kk   = U_k U_k^T - X_k^T Sigma_Sk         (15 x 15)
// and Sigma_SS of S_{k-1} = [k: 15][k+1: pose][k+2: pose] is Sigma_kk, the k+1 / k+2 pose rows of Sigma_Sk and the pose-pose
// part of the old Sigma_SS: the profile is closed under elimination, so nothing else is ever needed.  Only Sigma_SS is carried
// from step to step; the next keyframe's panel is fetched into registers while the current step computes.  Products on VALU
// from LDS: 11.4 us per step on one MI355X wave, latency-bound (DESIGN.md section 6) -- MFMA or register-resident operands are
// the way to a shorter step.
// Output per slot (View-sized array sig, SIG_SLOT doubles): Sigma_kk as its lower triangle (h_tri order), then Sigma_{k+1,k}
// (15 x 15 row-major, row = dof of k+1; zero for the window's last keyframe).  Windows whose sweep failed are left alone.
// depth > 0: the recursion stops after that many keyframes -- the blocks of the tail cost their own steps only, and are the bits of
// the whole-window call (each step reads what the steps behind it left, nothing in front).
constexpr int SI_LD = 16, SS_LD = 28;
constexpr int SI_ENT = 42 * 15;                    // panel entries used: 27 rows of B, 15 rows of U (the rhs row is not)
constexpr int SI_PF = (SI_ENT + 63) / 64;          // ... per lane
__global__ void __launch_bounds__(64) k_band_selinv(View v, const int* __restrict__ failed, double* __restrict__ sig, const int depth) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int lo = v.lo[w], hi = v.hi[w];
    if (hi - lo <= 0 || hi > v.M || lo < 0 || failed[w]) return;
    __shared__ double PB[27 * SI_LD], PU[15 * SI_LD], X[27 * SI_LD], SK[27 * SI_LD];
    __shared__ double SS[2][27 * SS_LD];
    for (int e = lane; e < 2 * 27 * SS_LD; e += 64) (&SS[0][0])[e] = 0.0;
    double pf[SI_PF];
    auto fetch = [&](int k) {
        const double* __restrict__ p = v.Lp + ((size_t)w * v.M + k) * PANEL;
#pragma unroll
        for (int t = 0; t < SI_PF; t++) {
            const int e = lane + 64 * t, r = e / 15, c = e - 15 * (e / 15);
            double x = 0.0;
            // rows of keyframes at or beyond hi are not part of the window: zero whatever the panel holds there
            if (e < SI_ENT && (r >= 27 || k + 1 + (r < 15 ? 0 : (r < 21 ? 1 : 2)) < hi)) x = p[panel_idx(r < 27 ? r : r + 1, c)];
            pf[t] = x;
        }
    };
    fetch(hi - 1);
    int cur = 0;
    const int stop = depth > 0 && hi - depth > lo ? hi - depth : lo;     // (the tail only: vf_engine_marginals_ex, VF_MARGINALS_TAIL)
    for (int k = hi - 1; k >= stop; k--) {
#pragma unroll
        for (int t = 0; t < SI_PF; t++) {
            const int e = lane + 64 * t, r = e / 15, c = e - 15 * (e / 15);
            if (e < SI_ENT) { if (r < 27) PB[r * SI_LD + c] = pf[t]; else PU[(r - 27) * SI_LD + c] = pf[t]; }
        }
        __syncthreads();
        if (k > lo) fetch(k - 1);
        // X = B U^T: U^T[m][j] = U[j][m], zero for m < j
        for (int e = lane; e < 27 * 15; e += 64) {
            const int i = e / 15, j = e - 15 * i;
            double s = 0.0;
            for (int m = j; m < 15; m++) s = fma(PB[i * SI_LD + m], PU[j * SI_LD + m], s);
            X[i * SI_LD + j] = s;
        }
        __syncthreads();
        const double* __restrict__ S0 = SS[cur];
        double* __restrict__ S1 = SS[cur ^ 1];
        for (int e = lane; e < 27 * 15; e += 64) {
            const int i = e / 15, j = e - 15 * i;
            double s = 0.0;
#pragma unroll 9
            for (int m = 0; m < 27; m++) s = fma(S0[i * SS_LD + m], X[m * SI_LD + j], s);
            SK[i * SI_LD + j] = -s;
        }
        __syncthreads();
        double* __restrict__ out = sig + ((size_t)w * v.M + k) * SIG_SLOT;
        for (int e = lane; e < 120; e += 64) {
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= e) a++;
            const int b = e - a * (a + 1) / 2;
            double s = 0.0;
            for (int m = a; m < 15; m++) s = fma(PU[a * SI_LD + m], PU[b * SI_LD + m], s);    // (U U^T)[a][b], a >= b
            for (int i = 0; i < 27; i++) s = fma(-X[i * SI_LD + a], SK[i * SI_LD + b], s);
            out[e] = s;
            S1[a * SS_LD + b] = s;
            S1[b * SS_LD + a] = s;
        }
        for (int e = lane; e < 225; e += 64) out[120 + e] = SK[(e / 15) * SI_LD + e % 15];
        // rows [k+1: pose] and [k+2: pose] of the new Sigma_SS: old index of new 15 + p is p, of new 21 + p is 15 + p
        for (int e = lane; e < 12 * 27; e += 64) {
            const int r = 15 + e / 27, c = e - 27 * (e / 27);
            const int orow = r < 21 ? r - 15 : r - 6;
            const double x = c < 15 ? SK[orow * SI_LD + c] : S0[orow * SS_LD + (c < 21 ? c - 15 : c - 6)];
            S1[r * SS_LD + c] = x;
            if (c < 15) S1[c * SS_LD + r] = x;
        }
        cur ^= 1;
        __syncthreads();
    }
}
void launch_band_factor(const View& v, const SolvePlan& plan, hipStream_t s) { launch_band_forward(v, plan.factor, s); }
void launch_selinv(const View& v, const int* failed, double* sig, int depth, hipStream_t s) {
    hipLaunchKernelGGL(k_band_selinv, dim3(v.B), dim3(64), 0, s, v, failed, sig, depth);
}
