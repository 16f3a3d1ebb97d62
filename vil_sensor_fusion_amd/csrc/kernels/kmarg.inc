// kernels/kmarg.inc -- fixed-lag marginalisation of the oldest keyframe (and its ahead-of-time form), the slide.
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// Fixed-lag marginalisation of the oldest keyframe m = lo (SURVEY 8f-3): the Schur complement of
// every factor touching m -- its prior or marginal prior, the IMU factor m -> m+1, the between
// factors starting at m -- taken at the current linearisation (buffer `sel`), onto
// [m+1: 15][m+2: pose 6][m+3: pose 6].  One 256-thread workgroup per window (1 024 threads in the big form), 42x42 system in LDS, Gaussian
// elimination of the 15 leading columns (no square roots).  Runs once per slide.
// stash != null (FAR = false only): the new marginal prior goes into stash[w][MARG_STASH] instead of the window's own arrays, and
// nothing of the window changes -- k_marg_commit puts it in place later (vf_engine_marginalize_ahead: the marginalisation a full
// fixed-lag window will need at its next update, computed behind the solve that has just finished instead of in front of the
// next one).
// FAR: 0 = the window holds no far factors; 1 = up to MAX_EXTRA of them, the joint system in LDS; 2 = up to MAX_EXTRA_BIG, the
// joint system in the window's View::far_scratch (engines made with max_far_factors > VF_MAX_EXTRA: the same arithmetic in
// the same order on the same numbers, so a window with eight or fewer far factors gets the same bits from either form).
constexpr int MARG_STASH = MARG_STASH_DOUBLES;
template <int FAR>
__global__ void __launch_bounds__(FAR == 2 ? 1024 : 256) k_marginalize(View v, int* status, double* __restrict__ stash) {
    constexpr int XC = FAR == 2 ? MAX_EXTRA_BIG : MAX_EXTRA;
    constexpr int NT = FAR == 2 ? 1024 : 256;        // threads of the workgroup (the big form is bound by the latency of its entry-parallel passes over device memory)
    const int w = blockIdx.x, lane = threadIdx.x;
    const int lo = v.lo[w], hi = v.hi[w];
    if (hi - lo < 4) { if (lane == 0) atomicOr(status, 2); return; }
    const int b = v.sel[w];
    const size_t tiles = (size_t)(v.G >> 6);
    const long g0 = (long)w * v.M + lo;
    __shared__ double A[42 * 43];
    __shared__ double bv[42];
    const double* imu = v.imu_r + (size_t)b * tiles * IMU_R * TILE + (size_t)((g0 + 1) >> 6) * IMU_R * TILE + ((g0 + 1) & 63);   // residual
    const double* jbuf = v.imu_j + (size_t)b * (size_t)(v.G >> JT_LOG) * JT_STRIDE;
    const bool has_prior = v.prior_k[w] == lo;
    const bool has_mp = v.mp_on[w] != 0;
    const double* Pq = v.prior_out + ((size_t)b * v.B + w) * PRIOR_OUT;
    const double* ML = v.mp_L + (size_t)w * 729;
    const double* Mg = v.mp_out + ((size_t)b * v.B + w) * 28;
    int bd[3];   // between factor m -> m+d present?
    for (int d = 1; d <= 3; d++) bd[d - 1] = (v.btw_a[g0 + d] == lo);
    // The linearisations of the factors that touch m are staged into LDS once (the whitened Jacobian of the IMU factor
    // m -> m+1 as a dense 15 x 30 block + its residual, the three between linearisations that may start at m); every
    // entry of the 42 x 42 system then costs LDS reads.  (Read where they lie -- J-stream entries through the index
    // table, AoSoA fields -- the 54 000 dependent global loads of this phase were most of the kernel's 95 us, i.e. an
    // eighth of a GraphManager solve.)
    __shared__ double LJ[15 * 30 + 15];
    __shared__ double LBt[3 * BTW_OUT];
    // far between factors that start at m and end within the prior's reach (m+1 .. m+3) are absorbed into the marginal prior
    // like band factors: a far factor is transported from keyframe to keyframe while its anchor leaves the window (vf_engine.hip
    // "transport_far") until it is this short, and its information then outlives both its ends
    __shared__ double LXt[XC * BTW_OUT];
    __shared__ int xd[XC];
    if (lane < XC) {
        int d = 0;
        if (lane < v.x_max) {
            const int i = w * v.x_max + lane, a = v.x_a[i], kb = v.x_b[i];
            if (a == lo && kb - lo >= 1 && kb - lo <= 3 && kb < hi) d = kb - lo;
        }
        xd[lane] = d;
    }
    __syncthreads();
    for (int e = lane; e < XC * BTW_OUT; e += NT) {
        const int s = e / BTW_OUT, f = e - s * BTW_OUT;
        LXt[e] = (s < v.x_max && xd[s]) ? v.x_out[(((size_t)b * v.B + w) * v.x_max + s) * BTW_OUT + f] : 0.0;
    }
    for (int e = lane; e < 15 * 30 + 15; e += NT)
        LJ[e] = e < 450 ? jstream_entry(jbuf, g0 + 1, e / 30, e % 30) : imu[(size_t)(e - 450) * TILE];
    for (int e = lane; e < 3 * BTW_OUT; e += NT) {
        const int d = e / BTW_OUT + 1, f = e - (d - 1) * BTW_OUT;
        const long gs = g0 + d;
        LBt[e] = bd[d - 1] ? v.btw_out[(size_t)b * tiles * BTW_OUT * TILE + ((size_t)(gs >> 6) * BTW_OUT + f) * TILE + (gs & 63)] : 0.0;
    }
    __syncthreads();
    auto JI = [&](int r, int c30) { return LJ[r * 30 + c30]; };
    // index maps of the 42-vector: [m:15][m+1:15][m+2 pose][m+3 pose]
    auto imu_c = [](int i) { return i < 15 ? imu_col(0, i) : imu_col(1, i - 15); };   // i < 30
    auto mp_i = [](int i) { return i < 15 ? i : (i < 21 ? i : (i >= 30 && i < 36 ? i - 9 : -1)); };   // 42-index -> 27-index
    for (int e = lane; e < 42 * 42 + 42; e += NT) {
        const bool is_b = e >= 42 * 42;
        const int i = is_b ? e - 42 * 42 : e / 42, j = is_b ? -1 : e - (e / 42) * 42;
        double sum = 0.0;
        if (i < 30 && (is_b || j < 30)) {   // IMU factor m -> m+1
            const int ci = imu_c(i);
            for (int r = 0; r < 15; r++) sum = fma(JI(r, ci), is_b ? LJ[450 + r] : JI(r, imu_c(j)), sum);
        }
        for (int q = 0; q < 3 + XC; q++) {      // between factors m -> m+d: Ja on m pose, Jb on (m+d) pose (band slots, then far slots)
            const int d = q < 3 ? (bd[q] ? q + 1 : 0) : xd[q - 3];
            if (!d) continue;
            const double* F = q < 3 ? LBt + q * BTW_OUT : LXt + (q - 3) * BTW_OUT;
            const int ob = d == 1 ? 15 : (d == 2 ? 30 : 36);
            const int ia = i < 6 ? i : -1, ib = (i >= ob && i < ob + 6) ? i - ob : -1;
            const int ja = (!is_b && j < 6) ? j : -1, jb = (!is_b && j >= ob && j < ob + 6) ? j - ob : -1;
            if (ia < 0 && ib < 0) continue;
            if (!is_b && ja < 0 && jb < 0) continue;
            for (int r = 0; r < 6; r++) {
                const double xi = ia >= 0 ? F[6 + r * 6 + ia] : F[42 + r * 6 + ib];
                const double xj = is_b ? F[r] : (ja >= 0 ? F[6 + r * 6 + ja] : F[42 + r * 6 + jb]);
                sum = fma(xi, xj, sum);
            }
        }
        if (has_prior && i < 15 && (is_b || j < 15))
            for (int r = 0; r < 15; r++) sum = fma(Pq[15 + r * 15 + i], is_b ? Pq[r] : Pq[15 + r * 15 + j], sum);
        if (has_mp) {
            const int mi = mp_i(i), mj = is_b ? 0 : mp_i(j);
            if (mi >= 0 && mj >= 0) sum += is_b ? Mg[mi] : ML[mi * 27 + mj];
        }
        if (is_b) bv[i] = sum; else A[i * 43 + j] = sum;
    }
    __syncthreads();
    // ---- FAR: the window's linear far factor (View::xl_*; every row of it has the leaving keyframe in its support) and the
    // nonlinear far factors anchored at m whose end lies beyond the prior's reach are marginalised WITH m, jointly and exactly
    // at the current linearisation.  With W = [W_mn | W_b | r] their whitened rows over (m and the prior's keyframes n: the 42
    // columns of A; the far ends b: 6 each; residual), the system to eliminate m from is
    //     [A + W_mn^T W_mn   (W_b^T W_mn)^T]         [bv + W_mn^T r]
    //     [W_b^T W_mn         W_b^T W_b    ]    and  [W_b^T r      ]
    // whose far-end rows are kept in E (the A block and bv in place).  A far end that has come within the prior's reach
    // (m + 3) is folded into the columns of that keyframe first.  After the 15 pivots, (n, b) hold the exact marginal S; it is
    // split again into a prior on n alone and six rows per far end:
    //     S_bb = L L^T,  X = L^-1 [S_bn | eta_b],  rows U' = [X_n | L^T], r' = x_eta;  prior: S_nn - X_n^T X_n, eta_n - X_n^T x_eta
    // (U'^T U' + prior = S).  Rows and far ends are written back compacted; the far ends' linearisation points move to the
    // current states, like the prior's.
    constexpr int FR = FAR ? 6 * XC : 1, FC = 42 + 6 * XC + 1;      // rows of W / E, their columns
    __shared__ double Wf_lds[FAR == 1 ? FR * FC : 1], E_lds[FAR == 1 ? FR * FC : 1];
    double* const Wf = FAR == 2 ? v.far_scratch + (size_t)w * FAR_SCRATCH : Wf_lds;
    double* const E = FAR == 2 ? Wf + (size_t)FR * FC : E_lds;
    __shared__ int f_kb[XC], f_src[XC], f_fold[XC], f_T, f_live;
    if constexpr (FAR) {
        const int nl_old = v.xl_n[w];
        if (lane == 0) {
            // far ends of the joint factor: the old linear ones, then the nonlinear far factors this marginalisation converts
            // (f_src: -1 - e = old far end e, i >= 0 = entry i of the nonlinear list)
            int T = 0;
            for (int e = 0; e < nl_old; e++) { f_kb[T] = v.xl_b[w * v.x_max + e]; f_src[T] = -1 - e; f_fold[T] = f_kb[T] == lo + 3; T++; }
            for (int i = 0; i < v.x_max && T < XC; i++) {
                const int a = v.x_a[w * v.x_max + i], kb = v.x_b[w * v.x_max + i];
                if (a == lo && kb - lo > 3 && kb < hi) { f_kb[T] = kb; f_src[T] = i; f_fold[T] = 0; T++; }
            }
            f_T = T;
        }
        __syncthreads();
        const int T = f_T, R = 6 * T, NC = 42 + 6 * T + 1;       // (columns: 0..41 as A, 42 + 6 t + c far end t, NC - 1 residual)
        for (int e = lane; e < R * FC; e += NT) {
            const int row = e / FC, c = e - row * FC, t = row / 6, j = row - 6 * t;
            double x = 0.0;
            if (c < NC) {
                const bool res = c == NC - 1;
                const int tc = (c >= 42 && !res) ? (c - 42) / 6 : -1, cc = tc >= 0 ? c - 42 - 6 * tc : 0;
                if (f_src[t] < 0) {
                    // row (6 e + j) of the old factor: columns [m: 0..14][m+1 pose: 15..20][m+2 pose: 21..26][far end q: 27 + 6 q ..]
                    const int eo = -1 - f_src[t];
                    const double* U = v.xl_U + ((size_t)w * 6 * v.x_max + 6 * eo + j) * xl_ld(v);
                    if (res) x = v.xl_out[((size_t)b * v.B + w) * 6 * v.x_max + 6 * eo + j];
                    else if (c < 21) x = U[c];                                     // m, pose of m + 1
                    else if (c >= 30 && c < 36) x = U[21 + c - 30];                // pose of m + 2
                    else if (tc >= 0 && f_src[tc] < 0) x = U[27 + 6 * (-1 - f_src[tc]) + cc];   // (old far ends keep their order: tc = that end)
                } else {
                    const double* F = v.x_out + (((size_t)b * v.B + w) * v.x_max + f_src[t]) * BTW_OUT;
                    if (res) x = F[j];
                    else if (c < 6) x = F[6 + j * 6 + c];
                    else if (tc == t) x = F[42 + j * 6 + cc];
                }
            }
            Wf[e] = x;
        }
        __syncthreads();
        // a far end at m + 3: its columns join the pose columns of that keyframe (36..41)
        for (int e = lane; e < R * 6; e += NT) {
            const int row = e / 6, c = e - row * 6;
            double add = 0.0;
            for (int t = 0; t < T; t++)
                if (f_fold[t]) { add += Wf[row * FC + 42 + 6 * t + c]; Wf[row * FC + 42 + 6 * t + c] = 0.0; }
            Wf[row * FC + 36 + c] += add;
        }
        __syncthreads();
        for (int e = lane; e < 42 * 43; e += NT) {
            const int i = e / 43, j = e - i * 43;
            double sum = 0.0;
            for (int r = 0; r < R; r++) sum = fma(Wf[r * FC + i], j < 42 ? Wf[r * FC + j] : Wf[r * FC + NC - 1], sum);
            if (j < 42) A[i * 43 + j] += sum; else bv[i] += sum;
        }
        if constexpr (FAR == 2) {
            // (W in device memory: its rows pass through LDS six at a time -- in LXt, free since the 42 x 42 system was formed --
            // and a thread forms eight entries at once; every entry the same chain of fma over r = 0 .. R - 1 as below)
            constexpr int CH = 6, ACC = 8;
            static_assert(CH * FC <= XC * BTW_OUT, "a chunk of W rows fits in LXt");
            double* const Wl = LXt;
            for (int e0 = 0; e0 < R * FC; e0 += NT * ACC) {
                double acc[ACC];
                int ip[ACC], ic[ACC];
#pragma unroll
                for (int i = 0; i < ACC; i++) {
                    const int e = e0 + i * NT + lane, p = e / FC, c = e - p * FC;
                    const bool live = e < R * FC && c < NC;
                    ip[i] = live ? 42 + p : 0;
                    ic[i] = live ? c : 0;
                    acc[i] = 0.0;
                }
                for (int r0 = 0; r0 < R; r0 += CH) {
                    __syncthreads();
                    for (int x = lane; x < CH * FC; x += NT) Wl[x] = Wf[r0 * FC + x];
                    __syncthreads();
#pragma unroll
                    for (int rr = 0; rr < CH; rr++)
#pragma unroll
                        for (int i = 0; i < ACC; i++) acc[i] = fma(Wl[rr * FC + ip[i]], Wl[rr * FC + ic[i]], acc[i]);
                }
#pragma unroll
                for (int i = 0; i < ACC; i++) {
                    const int e = e0 + i * NT + lane;
                    if (e < R * FC) E[e] = (e - (e / FC) * FC) < NC ? acc[i] : 0.0;
                }
            }
        } else {
            for (int e = lane; e < R * FC; e += NT) {
                const int p = e / FC, c = e - p * FC;
                double sum = 0.0;
                if (c < NC) for (int r = 0; r < R; r++) sum = fma(Wf[r * FC + 42 + p], Wf[r * FC + c], sum);
                E[e] = sum;
            }
        }
        __syncthreads();
    }
    int bad = 0;
    for (int c = 0; c < 15; c++) {
        const double d = A[c * 43 + c];
        if (!(d > 0.0)) bad = 1;
        const double inv = 1.0 / d;
        __syncthreads();
        // rank-1 update of the trailing (41-c)x(41-c) block and of b, entry-parallel; column c and
        // b[c] are only read in this step, so one pass is hazard-free
        const int m = 41 - c;
        for (int e = lane; e < m * m + m; e += NT) {
            const bool is_b = e >= m * m;
            const int i = c + 1 + (is_b ? e - m * m : e / m), j = is_b ? -1 : c + 1 + (e - (e / m) * m);
            const double u = A[i * 43 + c] * inv * (is_b ? bv[c] : A[j * 43 + c]);
            if (is_b) bv[i] -= u; else A[i * 43 + j] -= u;
        }
        if constexpr (FAR) {
            // the far-end rows: E[p][j] -= E[p][c] / d * (row c of the whole system)[j]; row c is A[c][.] over the 42 columns,
            // E[.][c] over the far-end columns (symmetry), bv[c] for the right-hand side
            const int R = 6 * f_T, NC = 42 + R + 1;
            for (int e = lane; e < R * FC; e += NT) {
                const int p = e / FC, j = e - p * FC;
                if (j <= c || j >= NC) continue;
                const double rc = j < 42 ? A[c * 43 + j] : (j < NC - 1 ? E[(j - 42) * FC + c] : bv[c]);
                E[e] -= E[p * FC + c] * inv * rc;
            }
        }
        __syncthreads();
    }
    if constexpr (FAR) {
        // ---- split the marginal over (n, far ends) into the prior on n and six rows per live far end
        const int T = f_T;
        if (lane == 0) { int L = 0; for (int t = 0; t < T; t++) if (!f_fold[t]) f_src[L++] = t; f_live = L; }    // (f_src: now the live far ends, in order)
        __syncthreads();
        const int Lv = f_live, RL = 6 * Lv;
        auto pr = [&](int q) { return 6 * f_src[q / 6] + q % 6; };              // live row / column q -> row of E (column 42 + that)
        // S_bb (live x live) -> Wf[q][q2] (row stride FC), then Cholesky in place, right-looking, entry-parallel
        for (int e = lane; e < RL * RL; e += NT) { const int q = e / RL, q2 = e - q * RL; Wf[q * FC + q2] = 0.5 * (E[pr(q) * FC + 42 + pr(q2)] + E[pr(q2) * FC + 42 + pr(q)]); }
        __syncthreads();
        // X = L^-1 [S_bn | eta_b] into Wf[q][RL + col], col = n's 27 columns (A's 15..41) and the right-hand side
        auto xsrc = [&](int col) { return col < 27 ? 15 + col : 42 + 6 * T; };
        if constexpr (FAR == 2) {
            // (device memory: the forward substitution rides on the factorisation -- pivot c scales column c of L, finishes row c of X and
            // takes L[q][c] X[c][.] off the rows below, so that row q has met k = 0 .. q - 1 in that order when its turn comes: the chain
            // of fma of the thread-per-column form below, without its 18 000 dependent loads)
            for (int e = lane; e < RL * 28; e += NT) { const int q = e / 28, col = e - q * 28; Wf[q * FC + RL + col] = E[pr(q) * FC + xsrc(col)]; }
            __syncthreads();
        }
        if constexpr (FAR == 2) {
            // NB pivots at a time: their columns of S (from the first pivot's row down) and their rows of X are factorised among
            // themselves in LDS (in LXt), then every entry below takes its NB updates in one visit to device memory -- the updates
            // an entry receives, their operands and their order are those of the step-by-step loop of the LDS form
            constexpr int NB = 8;
            static_assert(6 * XC * NB + NB * 28 <= XC * BTW_OUT, "panel and pivot rows of X fit in LXt");
            double* const Pn = LXt;                     // [rows][NB]
            double* const XP = LXt + 6 * XC * NB;       // [NB][28]
            for (int c0 = 0; c0 < RL; c0 += NB) {
                const int nb = min(NB, RL - c0), rows = RL - c0;
                __syncthreads();
                for (int e = lane; e < rows * nb; e += NT) { const int q = e / nb, j = e - q * nb; Pn[q * NB + j] = Wf[(c0 + q) * FC + c0 + j]; }
                for (int e = lane; e < nb * 28; e += NT) { const int j = e / 28, col = e - j * 28; XP[e] = Wf[(c0 + j) * FC + RL + col]; }
                __syncthreads();
                for (int j = 0; j < nb; j++) {
                    const double d = Pn[j * NB + j];
                    if (!(d > 0.0)) bad |= 4;            // (status bit 4: the far ends' block of the marginal is not positive definite)
                    const double sd = sqrt(d > 0.0 ? d : 1.0);
                    __syncthreads();
                    for (int q = j + lane; q < rows; q += NT) Pn[q * NB + j] = q == j ? sd : Pn[q * NB + j] / sd;
                    if (lane >= 228 && lane < 256) XP[j * 28 + lane - 228] = XP[j * 28 + lane - 228] / sd;
                    __syncthreads();
                    const int nj = nb - 1 - j, ns = (rows - 1 - j) * nj;
                    for (int e = lane; e < ns + nj * 28; e += NT) {
                        if (e < ns) {
                            const int q = j + 1 + e / nj, j2 = j + 1 + (e - (e / nj) * nj);
                            if (j2 <= q) Pn[q * NB + j2] -= Pn[q * NB + j] * Pn[j2 * NB + j];
                        } else {
                            const int x = e - ns, i = j + 1 + x / 28, col = x - (x / 28) * 28;
                            XP[i * 28 + col] = fma(-Pn[i * NB + j], XP[j * 28 + col], XP[i * 28 + col]);
                        }
                    }
                    __syncthreads();
                }
                for (int e = lane; e < rows * nb; e += NT) { const int q = e / nb, j = e - q * nb; if (j <= q) Wf[(c0 + q) * FC + c0 + j] = Pn[q * NB + j]; }
                for (int e = lane; e < nb * 28; e += NT) { const int j = e / 28, col = e - j * 28; Wf[(c0 + j) * FC + RL + col] = XP[e]; }
                const int tr = rows - nb, total = tr * tr + tr * 28;
                for (int e0 = 0; e0 < total; e0 += 4 * NT) {
                    double x[4];
                    int iq[4], ic[4];             // row (relative to c0); column: < 0 = none, [0, rows) = of S, rows + col = of X
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int e = e0 + u * NT + lane;
                        iq[u] = 0;
                        ic[u] = -1;
                        if (e < tr * tr) { const int q = nb + e / tr, q2 = nb + (e - (e / tr) * tr); if (q2 <= q) { iq[u] = q; ic[u] = q2; } }
                        else if (e < total) { const int y = e - tr * tr; iq[u] = nb + y / 28; ic[u] = rows + (y - (y / 28) * 28); }
                        x[u] = ic[u] < 0 ? 0.0 : Wf[(c0 + iq[u]) * FC + (ic[u] < rows ? c0 + ic[u] : RL + ic[u] - rows)];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (ic[u] < 0) continue;
                        if (ic[u] < rows) {
                            for (int j = 0; j < nb; j++) x[u] -= Pn[iq[u] * NB + j] * Pn[ic[u] * NB + j];
                            Wf[(c0 + iq[u]) * FC + c0 + ic[u]] = x[u];
                        } else {
                            const int col = ic[u] - rows;
                            for (int j = 0; j < nb; j++) x[u] = fma(-Pn[iq[u] * NB + j], XP[j * 28 + col], x[u]);
                            Wf[(c0 + iq[u]) * FC + RL + col] = x[u];
                        }
                    }
                }
            }
            __syncthreads();
        } else {
            for (int c = 0; c < RL; c++) {
                const double d = Wf[c * FC + c];
                if (!(d > 0.0)) bad |= 4;                // (status bit 4: the far ends' block of the marginal is not positive definite)
                const double sd = sqrt(d > 0.0 ? d : 1.0);
                __syncthreads();
                for (int q = c + lane; q < RL; q += NT) Wf[q * FC + c] = q == c ? sd : Wf[q * FC + c] / sd;
                __syncthreads();
                const int rem = RL - 1 - c;
                for (int e = lane; e < rem * rem; e += NT) {
                    const int q = c + 1 + e / rem, q2 = c + 1 + (e - (e / rem) * rem);
                    if (q2 <= q) Wf[q * FC + q2] -= Wf[q * FC + c] * Wf[q2 * FC + c];
                }
                __syncthreads();
            }
        }
        if (FAR != 2 && lane < 28) {
            const int src = xsrc(lane);
            for (int q = 0; q < RL; q++) {
                double a = E[pr(q) * FC + src];
                for (int k = 0; k < q; k++) a = fma(-Wf[q * FC + k], Wf[k * FC + RL + lane], a);
                Wf[q * FC + RL + lane] = a / Wf[q * FC + q];
            }
        }
        __syncthreads();
        // the prior on n loses what the rows now carry
        for (int e = lane; e < 27 * 28; e += NT) {
            const int i = e / 28, j = e - i * 28;
            double sum = 0.0;
            for (int q = 0; q < RL; q++) sum = fma(Wf[q * FC + RL + i], Wf[q * FC + RL + j], sum);
            if (j < 27) A[(15 + i) * 43 + 15 + j] -= sum; else bv[15 + i] -= sum;
        }
        // the rows: [X_n | L^T] over [n: 27][live far ends: 6 each], residual x_eta -- both buffers, the linearisation point
        // being the current states from here on
        const int ld = xl_ld(v);
        for (int e = lane; e < RL * ld; e += NT) {
            const int q = e / ld, c = e - q * ld;
            double x = 0.0;
            if (c < 27) x = Wf[q * FC + RL + c];
            else if (c - 27 < RL && c - 27 >= q) x = Wf[(c - 27) * FC + q];     // L^T: upper triangle
            v.xl_U[((size_t)w * 6 * v.x_max + q) * ld + c] = x;
        }
        for (int q = lane; q < 6 * v.x_max; q += NT) {
            const double x = q < RL ? Wf[q * FC + RL + 27] : 0.0;
            v.xl_r0[(size_t)w * 6 * v.x_max + q] = x;
            v.xl_out[((size_t)0 * v.B + w) * 6 * v.x_max + q] = x;
            v.xl_out[((size_t)1 * v.B + w) * 6 * v.x_max + q] = x;
        }
        __syncthreads();                                 // (xl_b is read through f_kb, written below)
        if (lane < Lv * 7) {
            const int q = lane / 7, c = lane - 7 * q;
            v.xl_bx[((size_t)w * v.x_max + q) * 7 + c] = XS(b, c, (long)w * v.M + f_kb[f_src[q]]);
        }
        if (lane >= 64 && lane < 64 + Lv) v.xl_b[w * v.x_max + lane - 64] = f_kb[f_src[lane - 64]];
        if (lane == 128) v.xl_n[w] = Lv;
        if (lane >= 192 && lane < 192 + v.x_max) {       // the nonlinear entries that have just become linear (the host re-sends the list without them)
            const int i = w * v.x_max + lane - 192;
            if (v.x_a[i] == lo && v.x_b[i] - lo > 3 && v.x_b[i] < hi) v.x_a[i] = -1;
        }
        __syncthreads();
    }
    // Gauge floor (vf_engine_opts.gauge_floor).  Every factor of the window is invariant under a global translation and a
    // rotation about gravity; what the window knows about those four directions is G^T L G of this prior alone -- the memory
    // of the anchor prior, which decays with every marginalisation until it is below the rounding of the 1e9-scale entries
    // beside it (cond(H) 5e12 after 100 updates of a 200-keyframe window, 1e16 after 2 000, indefinite after 3 000: LM trials
    // rejected at random, then failed solves).  Eigenvalues of G^T L G that have fallen below the floor are lifted back to it
    // (the default keeps the window's softest eigenvalue at 3e-4, two orders above the rounding of its largest entries: for
    // 1 000 keyframes an information of 0.1 on WHERE the window is, a 3 m sigma -- nothing the factors can see).
    if (v.gauge_floor > 0.0) {
        __shared__ double Gq[27 * 4], Tq[27 * 4], Mq[16], Vq[16], lift[4];
        for (int e = lane; e < 729; e += NT) {          // the symmetric part, in place
            const int i = e / 27, j = e - i * 27;
            if (j > i) { const double sy = 0.5 * (A[(15 + i) * 43 + 15 + j] + A[(15 + j) * 43 + 15 + i]); A[(15 + i) * 43 + 15 + j] = sy; A[(15 + j) * 43 + 15 + i] = sy; }
        }
        for (int e = lane; e < 108; e += NT) Gq[e] = 0.0;
        __syncthreads();
        if (lane < 3) {                                  // lane j: the rows of kept keyframe j
            const int j = lane, o = j == 0 ? 0 : 15 + 6 * (j - 1);
            const State s0 = load_state(v, b, g0 + 1), sj = load_state(v, b, g0 + 1 + j);
            const M3 R = qrot(sj.q);
            const double gn = sqrt(v.grav[0] * v.grav[0] + v.grav[1] * v.grav[1] + v.grav[2] * v.grav[2]);
            const V3 ez = gn > 0.0 ? v3(-v.grav[0] / gn, -v.grav[1] / gn, -v.grav[2] / gn) : v3(0.0, 0.0, 1.0);
            const V3 dt = sj.t - s0.t;
            const V3 lever = v3(ez.y * dt.z - ez.z * dt.y, ez.z * dt.x - ez.x * dt.z, ez.x * dt.y - ez.y * dt.x);
            for (int c = 0; c < 3; c++) {
                for (int a = 0; a < 3; a++) Gq[(o + 3 + c) * 4 + a] = R.a[a * 3 + c];
                Gq[(o + c) * 4 + 3] = R.a[0 * 3 + c] * ez.x + R.a[1 * 3 + c] * ez.y + R.a[2 * 3 + c] * ez.z;
                Gq[(o + 3 + c) * 4 + 3] = R.a[0 * 3 + c] * lever.x + R.a[1 * 3 + c] * lever.y + R.a[2 * 3 + c] * lever.z;
            }
            if (j == 0) {
                Gq[6 * 4 + 3] = ez.y * sj.vel.z - ez.z * sj.vel.y;
                Gq[7 * 4 + 3] = ez.z * sj.vel.x - ez.x * sj.vel.z;
                Gq[8 * 4 + 3] = ez.x * sj.vel.y - ez.y * sj.vel.x;
            }
        }
        __syncthreads();
        if (lane == 0) {                                 // modified Gram-Schmidt, 4 columns of 27
            for (int a = 0; a < 4; a++) {
                for (int bb = 0; bb < a; bb++) {
                    double s = 0.0;
                    for (int i = 0; i < 27; i++) s += Gq[i * 4 + a] * Gq[i * 4 + bb];
                    for (int i = 0; i < 27; i++) Gq[i * 4 + a] -= s * Gq[i * 4 + bb];
                }
                double nn = 0.0;
                for (int i = 0; i < 27; i++) nn += Gq[i * 4 + a] * Gq[i * 4 + a];
                nn = sqrt(nn);
                for (int i = 0; i < 27; i++) Gq[i * 4 + a] /= nn;
            }
        }
        __syncthreads();
        if (lane < 108) {
            const int i = lane >> 2, a = lane & 3;
            double s = 0.0;
            for (int j = 0; j < 27; j++) s += A[(15 + i) * 43 + 15 + j] * Gq[j * 4 + a];
            Tq[lane] = s;
        }
        __syncthreads();
        if (lane < 16) {
            const int a = lane >> 2, bb = lane & 3;
            double s = 0.0;
            for (int i = 0; i < 27; i++) s += Gq[i * 4 + a] * Tq[i * 4 + bb];
            Mq[lane] = s;
        }
        __syncthreads();
        if (lane == 0) {                                 // cyclic Jacobi on the 4 x 4 (10 sweeps)
            for (int a = 0; a < 4; a++)
                for (int bb = a + 1; bb < 4; bb++) { const double sy = 0.5 * (Mq[a * 4 + bb] + Mq[bb * 4 + a]); Mq[a * 4 + bb] = sy; Mq[bb * 4 + a] = sy; }
            for (int i = 0; i < 16; i++) Vq[i] = (i % 5 == 0) ? 1.0 : 0.0;
            for (int sweep = 0; sweep < 10; sweep++)
                for (int p = 0; p < 3; p++)
                    for (int q = p + 1; q < 4; q++) {
                        const double apq = Mq[p * 4 + q];
                        if (apq == 0.0) continue;
                        const double theta = (Mq[q * 4 + q] - Mq[p * 4 + p]) / (2.0 * apq);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                        for (int kk = 0; kk < 4; kk++) {
                            const double mkp = Mq[kk * 4 + p], mkq = Mq[kk * 4 + q];
                            Mq[kk * 4 + p] = c * mkp - sn * mkq;
                            Mq[kk * 4 + q] = sn * mkp + c * mkq;
                            const double vkp = Vq[kk * 4 + p], vkq = Vq[kk * 4 + q];
                            Vq[kk * 4 + p] = c * vkp - sn * vkq;
                            Vq[kk * 4 + q] = sn * vkp + c * vkq;
                        }
                        for (int kk = 0; kk < 4; kk++) {
                            const double mpk = Mq[p * 4 + kk], mqk = Mq[q * 4 + kk];
                            Mq[p * 4 + kk] = c * mpk - sn * mqk;
                            Mq[q * 4 + kk] = sn * mpk + c * mqk;
                        }
                    }
            // (the floor is set on the WINDOW's eigenvalue: a unit gauge vector of an n-keyframe window has 3 / n of its weight
            // on the three keyframes this prior touches)
            const double floor_p = v.gauge_floor * (double)(v.hi[w] - v.lo[w]) / 3.0;
            for (int e = 0; e < 4; e++) { const double l = floor_p - Mq[e * 4 + e]; lift[e] = l > 0.0 ? l : 0.0; }
        }
        __syncthreads();
        if (lane < 108) {                                // q_e = G V[:, e]
            const int i = lane >> 2, e = lane & 3;
            double s = 0.0;
            for (int a = 0; a < 4; a++) s += Gq[i * 4 + a] * Vq[a * 4 + e];
            Tq[lane] = s;
        }
        __syncthreads();
        for (int e = lane; e < 729; e += NT) {
            const int i = e / 27, j = e - i * 27;
            double add = 0.0;
            for (int q = 0; q < 4; q++) add += lift[q] * Tq[i * 4 + q] * Tq[j * 4 + q];
            A[(15 + i) * 43 + 15 + j] += add;
        }
        __syncthreads();
    }
    // new marginal prior on [m+1:15][m+2 pose][m+3 pose] = rows 15..41, relinearised at the current states
    if (!FAR && stash) {
        double* st = stash + (size_t)w * MARG_STASH;
        for (int e = lane; e < 729 + 27; e += NT) {
            if (e < 729) { const int i = e / 27, j = e - i * 27; st[e] = 0.5 * (A[(15 + i) * 43 + 15 + j] + A[(15 + j) * 43 + 15 + i]); }
            else st[e] = bv[15 + e - 729];
        }
        if (lane < 48) { const int j = lane / 16, c = lane - j * 16; st[756 + lane] = XS(b, c, g0 + 1 + j); }
        if (lane == 0 && bad) atomicOr(status, bad & 4 ? 4 : 1);
        return;
    }
    for (int e = lane; e < 729 + 27; e += NT) {
        if (e < 729) { const int i = e / 27, j = e - i * 27; v.mp_L[(size_t)w * 729 + e] = 0.5 * (A[(15 + i) * 43 + 15 + j] + A[(15 + j) * 43 + 15 + i]); }
        else {
            // also the "linearised" form at the new linearisation point (d = 0: gradient eta, cost 0),
            // so that a second marginalisation can follow without an intervening linearise
            const double et = bv[15 + e - 729];
            v.mp_eta[(size_t)w * 27 + e - 729] = et;
            v.mp_out[((size_t)0 * v.B + w) * 28 + e - 729] = et;
            v.mp_out[((size_t)1 * v.B + w) * 28 + e - 729] = et;
        }
    }
    if (lane == 0) { v.mp_out[((size_t)0 * v.B + w) * 28 + 27] = 0.0; v.mp_out[((size_t)1 * v.B + w) * 28 + 27] = 0.0; }
    if (lane < 48) { const int j = lane / 16, c = lane - j * 16; v.mp_x[(size_t)w * 48 + lane] = XS(b, c, g0 + 1 + j); }
    if (lane == 0) {
        v.mp_on[w] = 1;
        v.prior_k[w] = -1;
        if (bad) atomicOr(status, bad & 4 ? 4 : 1);
    }
}

// what k_marginalize (stash != null) computed ahead of time becomes the window's marginal prior, exactly as the kernel itself
// would have left it
__global__ void __launch_bounds__(256) k_marg_commit(View v, const double* __restrict__ stash) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const double* st = stash + (size_t)w * MARG_STASH;
    for (int e = lane; e < 729 + 27; e += 256) {
        if (e < 729) v.mp_L[(size_t)w * 729 + e] = st[e];
        else {
            const double et = st[e];
            v.mp_eta[(size_t)w * 27 + e - 729] = et;
            v.mp_out[((size_t)0 * v.B + w) * 28 + e - 729] = et;
            v.mp_out[((size_t)1 * v.B + w) * 28 + e - 729] = et;
        }
    }
    if (lane == 0) { v.mp_out[((size_t)0 * v.B + w) * 28 + 27] = 0.0; v.mp_out[((size_t)1 * v.B + w) * 28 + 27] = 0.0; }
    if (lane < 48) v.mp_x[(size_t)w * 48 + lane] = st[756 + lane];
    if (lane == 0) {
        v.mp_on[w] = 1;
        v.prior_k[w] = -1;
    }
}

// fixed-lag slide by one keyframe: hi += 1 (predict the new state), lo += 1, and either re-anchor
// the diagonal prior on the new oldest keyframe (reanchor = 1) or keep the marginal prior that
// k_marginalize just produced (reanchor = 0)
__global__ void k_slide(View v, const double* sigma15, int reanchor) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= v.B) return;
    const int b = v.sel[w];
    const int hi = v.hi[w], lo = v.lo[w];
    if (hi >= v.M) return;  // out of slots: caller must compact
    const long gnew = (long)w * v.M + hi;
    store_state(v, b, gnew, predict_state(v, load_state(v, b, gnew - 1), gnew));
    v.hi[w] = hi + 1;
    v.lo[w] = lo + 1;
    if (!reanchor) return;
    const long ganchor = (long)w * v.M + lo + 1;
    v.prior_k[w] = lo + 1;
    v.mp_on[w] = 0;
    double* pin = v.prior_in + (size_t)w * PRIOR_IN;
    for (int c = 0; c < 16; c++) pin[c] = XS(b, c, ganchor);
    for (int c = 0; c < 15; c++) pin[16 + c] = sigma15[c];
}
