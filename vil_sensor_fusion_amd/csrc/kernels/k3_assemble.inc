// kernels/k3_assemble.inc -- K3: block-banded J^T J / J^T r on the matrix cores, owner-computes per keyframe.
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ K3
// Block-sparse J^T J / J^T r, owner-computes per keyframe, deterministic (no atomics):
//   H[k][k]   = Jj^T Jj (imu k) + Ji^T Ji (imu k+1) + between (as b at k, as a at k+d) + prior
//   H[k][k-1] = Jj^T Ji (imu k) + Jb^T Ja (between a=k-1)
//   H[k][k-d] = Jb^T Ja (between a=k-d), pose 6x6 only
// One 256-thread block per tile of 16 keyframes.  The tile's 17 IMU linearisations (r | J) are
// staged once into LDS with coalesced 128-byte segments (every J entry leaves HBM exactly once),
// then each wave forms the 16x16 blocks of [J r]^T [J r] for 4 keyframes with
// v_mfma_f64_16x16x4 (column 15 of a tile carries J^T r, so the gradient comes for free) and
// writes the H block rows coalesced straight from the MFMA C layout.  The 6x6 between terms and
// the prior are added on the VALU from LDS before the store.
// structural zeros of the whitened 15x30 IMU Jacobian (k_linearize_imu never writes them, the buffers are zero-filled
// at creation): field f = 15 + 30 r + c of a factor's (r | J) record
__host__ __device__ constexpr bool imu_field_is_zero(int f) {
    if (f < 15 || f >= IMU_OUT) return false;
    const int r = (f - 15) / 30, c = (f - 15) % 30;
    if (c < 18) return r >= 9 || (c >= 3 && c < 6 && r >= 6) || (c >= 12 && c < 15 && r > 3 + (c - 12));
    return r >= 10 + (c - 18) % 6;
}
// bit b of word w: field 32 w + b of a factor's (r | J) record exists and is not a structural zero
__host__ __device__ constexpr unsigned imu_nz_word(int w) {
    unsigned m = 0;
    for (int bit = 0; bit < 32; bit++) {
        const int f = 32 * w + bit;
        if (f < IMU_OUT && !imu_field_is_zero(f)) m |= 1u << bit;
    }
    return m;
}
constexpr int AT = JT;         // keyframes per block (one tile of the J stream)
constexpr int K3_NT = 256;     // threads per block
constexpr int K3_KPW = AT / (K3_NT / 64);   // keyframes per wave
static_assert(K3_KPW * (K3_NT / 64) == AT && K3_NT % AT == 0, "K3 tiling");
constexpr int LBS = 79;         // LDS stride of one between linearisation (78 + pad), odd

#ifdef VF_SOLVE_STAMPS   // diagnostic build only: phase time stamps of one workgroup of K3 (tools/k3_stamps_probe.py)
__device__ unsigned long long g_k3_stamps[8];
#define K3STAMP(i) do { if (blockIdx.x == 40 && blockIdx.y == (gridDim.y >> 1) && threadIdx.x == 0) { unsigned long long _t; asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t) :: "memory"); g_k3_stamps[i] = _t; } } while (0)
#else
#define K3STAMP(i) do {} while (0)
#endif
#ifdef VF_SOLVE_STAMPS
__device__ unsigned long long g_k3_loop[8];
#define K3LOOP(i) do { __builtin_amdgcn_sched_barrier(0); unsigned long long _t; asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t) :: "memory"); __builtin_amdgcn_sched_barrier(0); k3acc[i] += _t - k3prev; k3prev = _t; } while (0)
#else
#define K3LOOP(i) do {} while (0)
#endif
// Per-lane operand maps of assemble_tile and the window scalars it needs.  They come from memory (the index table of the J
// stream, per-window flags): the caller builds them while its staging loads are in flight, not behind the barrier that
// follows them -- two dependent round trips (about 3 k cycles per tile) taken off the matrix-core phase.
struct AsmMaps { int offI[4], offJ[4], oA[2], oB[2], prior_key; bool marg_on; };
__device__ __forceinline__ AsmMaps make_asm_maps(const View& v, const int w, const int lo, const int hi, const int lane) {
    AsmMaps m;
    const int ci = lane & 15, kq = lane >> 4;
    int (&offI)[4] = m.offI, (&offJ)[4] = m.offJ, (&oA)[2] = m.oA, (&oB)[2] = m.oB;
    // MFMA operand words of this lane in a factor's LDS image: J[4 q + kq][column ci of the i / j side], column 15 = r;
    // structural zeros and the padding row 15 read the zero cell
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int row = 4 * q + kq;
        offI[q] = offJ[q] = LJ_ZERO;
        if (row < 15) {
            if (ci < 15) {
                const int eI = JMD.idx[row * 30 + imu_col(0, ci)], eJ = JMD.idx[row * 30 + imu_col(1, ci)];
                if (eI >= 0) offI[q] = eI;
                if (eJ >= 0) offJ[q] = 2 * JS_PI + eJ;
            } else offI[q] = offJ[q] = LJ_R + row;
        }
    }
    // Between-factor terms on the matrix cores as well: a between linearisation in LDS (r: 0, Ja: 6, Jb: 42, 6 rows) is
    // the 6 x 16 operand X = [J | 0 ... 0 | r] (column 15 = r, like the IMU tiles), rows padded to 8 = two k-steps;
    // X^T X adds J^T J to the pose block and J^T r to the gradient column of a diagonal tile, Xb^T Xa is the coupling
    // block.  Per lane: the in-slot offsets of its two operand words (the slot's pad cell = 0 where X has no entry).
    // (the VALU form, 6-term dot products per entry from LDS, cost 0.5 ms of K3's 2.7; this one about 0.35)
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int row = 4 * q + kq;
        const bool valid = row < 6;
        oA[q] = !valid ? BTW_OUT : (ci < 6 ? 6 + row * 6 + ci : (ci == 15 ? row : BTW_OUT));
        oB[q] = !valid ? BTW_OUT : (ci < 6 ? 42 + row * 6 + ci : (ci == 15 ? row : BTW_OUT));
    }
    m.prior_key = v.prior_k[w];
    m.marg_on = v.mp_on[w] != 0 && hi - lo >= 3;
    return m;
}
// The matrix-core part of K3: wave `wv` of the workgroup forms the block rows of KPW keyframes from the tile's (r | J) rows in LJ and the
// between linearisations in LB (s_a = their source keyframes), and stores them into H, g.
template <int KPW>
__device__ __forceinline__ void assemble_tile(const View& v, const double* __restrict__ LJ, const double* __restrict__ LB,
                                              const int* __restrict__ s_a, const int w, const int b, const int k0,
                                              const long gk0, const int lo, const int hi, const int rlo, const int rhi,
                                              const int wv, const int lane, const AsmMaps& maps) {
    const int ci = lane & 15, kq = lane >> 4;
    const int (&offI)[4] = maps.offI, (&offJ)[4] = maps.offJ, (&oA)[2] = maps.oA, (&oB)[2] = maps.oB;
    auto load_ops = [&](int lf, double (&ai)[4], double (&aj)[4]) {
        const double* F = LJ + lf * LJS;
#pragma unroll
        for (int q = 0; q < 4; q++) { ai[q] = F[offI[q]]; aj[q] = F[offJ[q]]; }
    };
#ifdef VF_SOLVE_STAMPS
    unsigned long long k3acc[8] = {0}, k3prev = __builtin_amdgcn_s_memtime();
#endif
    // (window-level scalars: read by the caller in front of its staging barrier -- a global load inside the loop would have
    // to wait for its result with s_waitcnt vmcnt(0), and stores count in vmcnt on this ISA)
    const int prior_key = maps.prior_key;
    const bool marg_on = maps.marg_on;
    d4_t D = {0, 0, 0, 0};
    const int lf0 = KPW * wv;
#pragma unroll 1
    for (int lf = lf0; lf <= lf0 + KPW; lf++) {
        K3LOOP(0);
        double ai[4], aj[4];
        load_ops(lf, ai, aj);
        K3LOOP(1);    // operands of factor lf in registers
        if (lf > lf0) {
            // ---- finish keyframe kf = lf-1: D += Ji^T Ji of factor lf, add 6x6 terms, store
#pragma unroll
            for (int q = 0; q < 4; q++) D = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[q], ai[q], D, 0, 0, 0);
            K3LOOP(2);    // Ji^T Ji issued
            const int kl = lf - 1, k = k0 + kl;
            if (k >= rlo && k < rhi) {
                const long gk = gk0 + kl;
                double* Hk = v.H + (size_t)gk * HROW;
                // (accumulated into D itself: separate accumulators added at the end measured 4 % slower)
                if (__builtin_amdgcn_readfirstlane(s_a[kl]) >= 0) {   // a between factor ends here: Jb^T [Jb | r]
                    const double x0 = LB[kl * LBS + oB[0]], x1 = LB[kl * LBS + oB[1]];
                    D = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x0, D, 0, 0, 0);
                    D = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x1, D, 0, 0, 0);
                }
#pragma unroll
                for (int d = 1; d <= 3; d++)
                    if (__builtin_amdgcn_readfirstlane(s_a[kl + d]) == k) {   // ... or starts here: Ja^T [Ja | r]
                        const double x0 = LB[(kl + d) * LBS + oA[0]], x1 = LB[(kl + d) * LBS + oA[1]];
                        D = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x0, D, 0, 0, 0);
                        D = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x1, D, 0, 0, 0);
                    }
                const bool is_prior = prior_key == k;
                const double* Pq = v.prior_out + ((size_t)b * v.B + w) * PRIOR_OUT;
                const int mo = marg_on ? k - lo : 99;   // 0,1,2: rows of the marginal prior
                const double* ML = v.mp_L + (size_t)w * 729;
                const double* Mg = v.mp_out + ((size_t)b * v.B + w) * 28;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int a = kq + 4 * r;
                    double val = D[r];
                    if (is_prior && a < 15) {
                        double sum = 0.0;
                        for (int rr = 0; rr < 15; rr++)
                            sum = fma(Pq[15 + rr * 15 + a], ci < 15 ? Pq[15 + rr * 15 + ci] : Pq[rr], sum);
                        val += sum;
                    }
                    if (mo == 0 && a < 15) val += ci < 15 ? ML[a * 27 + ci] : Mg[a];
                    if ((mo == 1 || mo == 2) && a < 6 && (ci < 6 || ci == 15)) {
                        const int ob = mo == 1 ? 15 : 21;
                        val += ci < 6 ? ML[(ob + a) * 27 + ob + ci] : Mg[ob + a];
                    }
                    if (a < 15) {
                        if (ci <= a) __builtin_nontemporal_store(val, Hk + H_D0 + h_tri(a, ci));   // lower triangle only
                        else if (ci == 15) v.gvec[(size_t)gk * 15 + a] = val;
                    }
                }
            }
        }
        K3LOOP(3);        // diagonal tile finished and stored
        if (lf < lf0 + KPW) {
            // ---- keyframe kf = lf: off-diagonal block Jj^T Ji, pose-only blocks, start D = Jj^T Jj
            d4_t O = {0, 0, 0, 0};
            D = (d4_t){0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                O = __builtin_amdgcn_mfma_f64_16x16x4f64(aj[q], ai[q], O, 0, 0, 0);
                D = __builtin_amdgcn_mfma_f64_16x16x4f64(aj[q], aj[q], D, 0, 0, 0);
            }
            const int kl = lf, k = k0 + kl;
            if (k >= rlo && k < rhi) {
                double* Hk = v.H + (size_t)(gk0 + kl) * HROW;
                const int ak = __builtin_amdgcn_readfirstlane(s_a[kl]);
                const int dk = ak >= 0 ? k - ak : 0;   // 1..3 when a between factor ends here
                const int mo2 = marg_on ? k - lo : 99;
                const double* ML2 = v.mp_L + (size_t)w * 729;
                d4_t T = {0, 0, 0, 0};                    // Jb^T Ja of the between factor ending here
                if (dk >= 1) {
                    const double b0 = LB[kl * LBS + oB[0]], b1 = LB[kl * LBS + oB[1]];
                    const double a0 = LB[kl * LBS + oA[0]], a1 = LB[kl * LBS + oA[1]];
                    T = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, a0, T, 0, 0, 0);
                    T = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, a1, T, 0, 0, 0);
                }
                if (k > lo) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int a = kq + 4 * r;
                        double val = O[r];
                        if (dk == 1 && a < 6 && ci < 6) val += T[r];
                        if (mo2 == 1 && a < 6 && ci < 15) val += ML2[(15 + a) * 27 + ci];            // (lo+1 pose) x (lo: 15)
                        if (mo2 == 2 && a < 6 && ci < 6) val += ML2[(21 + a) * 27 + 15 + ci];        // (lo+2 pose) x (lo+1 pose)
                        if (a < 15 && ci < 15) __builtin_nontemporal_store(val, Hk + H_D1 + a * 15 + ci);
                    }
                }
                // pose x pose blocks two and three keyframes back, straight from the MFMA C layout (rows kq + 4 r)
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    const int a6 = kq + 4 * r;
                    if (a6 < 6 && ci < 6) {
                        const double x = T[r];
                        Hk[H_D2 + a6 * 6 + ci] = (dk == 2 ? x : 0.0) + (mo2 == 2 ? ML2[(21 + a6) * 27 + ci] : 0.0);
                        Hk[H_D3 + a6 * 6 + ci] = dk == 3 ? x : 0.0;
                    }
                }
                // the marginal prior couples (lo+2 pose) with all 15 dof of lo: columns 6..14 of the
                // d=2 strip (the solver reads them only for the window's third keyframe)
                if (mo2 == 2 && lane < 54) {
                    const int a6 = lane / 9, b9 = 6 + lane - a6 * 9;
                    Hk[H_DX + a6 * 9 + (b9 - 6)] = ML2[(21 + a6) * 27 + b9];
                }
            }
        }
    }
    K3LOOP(4);        // off-diagonal part
#ifdef VF_SOLVE_STAMPS
    if (blockIdx.x == 40 && blockIdx.y == (gridDim.y >> 1) && threadIdx.x == 0) for (int i = 0; i < 8; i++) g_k3_loop[i] = k3acc[i];
#endif
}

// Four waves per SIMD (128 VGPRs) = four workgroups per CU, which is also what the 40 KB of LDS allow: 2.23 -> 1.98 ms once
// the staging code had come down to 132 VGPRs (at 176 it spilled and lost).
__attribute__((amdgpu_waves_per_eu(4, 4)))
__global__ void __launch_bounds__(K3_NT) k_assemble(View v) {
    __shared__ __attribute__((aligned(16))) double LJ[(AT + 1) * LJS];
    __shared__ double LB[(AT + 3) * LBS];
    __shared__ int s_a[AT + 3];
    const int tid = threadIdx.x;
    // grid = (tiles per window, windows).  A rejected LM trial leaves the current linearisation, hence H and g,
    // unchanged (k_decide clears `fresh` on reject; accept / init / slide set it): such a tile must cost as little
    // as a launch can -- one flag read, no index arithmetic in front of it (an all-rejected batch used to take 0.73 ms)
    const int w = blockIdx.y + v.w_first;
    // (the window's scalars requested together, in front of the first test: one memory round trip, not three)
    // (hybrid solve of an engine whose sweep assembles its own rows: K3 works for the partitioned form only -- launched with
    // gate = 2, it returns while the sweep is the form in charge, and when it does run it cannot trust `fresh`: the trials the
    // sweep served never brought H up to date)
    const int fr = (v.gate == 2 || v.inc_on) ? 1 : v.fresh[w], lo = v.lo[w], hi = v.hi[w], w_sel = v.sel[w], w_done = v.stop_on ? v.done[w] : 0;
    const int ik = v.inc_on ? v.inc_k[w] : 0;
    if (!fr || w_done || gated_off(v)) return;
    const int k0 = blockIdx.x * AT;
    const long gk0 = (long)w * v.M + k0;
    // incremental update: a factor reaches three keyframes back, so the rows from inc_k - 3 on are new -- all of them when
    // the sweep starts at the window's first keyframe (the head rows carry the marginal prior of the last slide)
    const int inc_rlo = (v.inc_on && inc_start(ik, lo) > lo) ? ik - 3 : lo;
    if (k0 + AT <= inc_rlo) return;
    // warm start (k_linearize_tail): fr = 1 + appended keyframes; only rows near the ends of the window changed --
    // head: the marginal prior / the factors that left with the oldest keyframe reach rows lo .. lo+3;
    // tail: a new factor at slot b touches rows b-3 .. b
    if (fr >= 2 && fr < 64 && k0 >= lo + 4 && k0 + AT <= hi - (fr - 1) - 4) return;
    int rlo, rhi;                            // rows of H this rank assembles (absolute slots)
    own_range(v, w, rlo, rhi);
    rlo += lo;
    rhi += lo;
    if (v.sh_G > 1 && rhi + 2 <= hi) rhi += 2;   // tail rows of the rank's last chunk (see shard_skips_factor)
    else if (v.sh_G > 1) rhi = hi;
    rlo = rlo > inc_rlo ? rlo : inc_rlo;
    if (k0 + AT <= rlo || k0 >= rhi) return; // no owned active keyframe in this tile (uniform)
    K3STAMP(0);
    const int b = w_sel;
    const size_t tiles = (size_t)(v.G >> 6);
    const double* btw_out = v.btw_out + (size_t)b * tiles * BTW_OUT * TILE;

    AsmMaps maps;
    // ---- stage the tile's 9 IMU linearisations from the J stream: the tile's own block is copied into LDS as it is
    // (146 pairs x 8 slots, 16 bytes per lane and load, every 128-B line used whole, one ds_write_b128 each), the i-side
    // pairs of the halo factor come from slot 0 of the next tile.  All of a thread's global loads are issued before the
    // first LDS write.
    {
        constexpr int NOWN = JS_PAIRS * JT, NALL = NOWN + JS_PI, NJ = (NALL + K3_NT - 1) / K3_NT,
                      NB = ((AT + 3) * BTW_OUT + K3_NT - 1) / K3_NT;
        static_assert(AT == JT, "K3 tiles are the tiles of the J stream");
        const d2_t* jt = (const d2_t*)(v.imu_j + ((size_t)b * (size_t)(v.G >> JT_LOG) + (size_t)(gk0 >> JT_LOG)) * JT_STRIDE);
        const bool halo_ok = k0 + AT > lo && k0 + AT < hi;          // (then the next tile exists: k0 + AT < M)
        d2_t tj[NJ];
#pragma unroll
        for (int it = 0; it < NJ; it++) {
            const int e = it * K3_NT + tid;
            const int src = e < NOWN ? e : (e < NALL && halo_ok ? NOWN + (e - NOWN) * JT : 0);   // halo: pair p of slot 0 of the next tile
            tj[it] = jt[src];
        }
        // residuals of the 9 factors: 135 words
        double tr = 0.0;
        if (tid < (AT + 1) * IMU_R) {
            const int fac = tid / IMU_R, a = tid - fac * IMU_R;
            const long gf = gk0 + fac;
            const int kf = k0 + fac;
            if (kf > lo && kf < hi) tr = v.imu_r[((size_t)b * tiles + (size_t)(gf >> 6)) * IMU_R * TILE + (size_t)a * TILE + (gf & 63)];
        }
        // between linearisations of slots k0 .. k0+10
        double tb[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int e = tid + K3_NT * j;
            const int sl = e / BTW_OUT, f = e - sl * BTW_OUT;
            const int ks = k0 + sl;
            const long gs = gk0 + sl;
            tb[j] = (e < (AT + 3) * BTW_OUT && ks > lo && ks < hi) ? btw_out[((size_t)(gs >> 6) * BTW_OUT + f) * TILE + (gs & 63)] : 0.0;
        }
        K3STAMP(1);   // all loads issued
        maps = make_asm_maps(v, w, lo, hi, tid & 63);      // (their table / flag reads fly with the staging loads)
        if (tid < AT + 3) {
            LB[tid * LBS + BTW_OUT] = 0.0;       // the pad cell of a slot: the zero the MFMA operand maps point at
            const int ks = k0 + tid;
            int a = -1;
            if (ks > lo && ks < hi) { a = v.btw_a[gk0 + tid]; if (a < lo || a >= ks) a = -1; }
            s_a[tid] = a;
        }
        if (tid <= AT) LJ[tid * LJS + LJ_ZERO] = 0.0;
        if (tid < (AT + 1) * IMU_R) LJ[(tid / IMU_R) * LJS + LJ_R + tid % IMU_R] = tr;
#pragma unroll
        for (int it = 0; it < NJ; it++) {
            const int e = it * K3_NT + tid;
            if (e < NALL) {
                const int own = e < NOWN;
                const int pr = own ? e >> JT_LOG : e - NOWN;
                const int fac = own ? e & (JT - 1) : AT;
                const int kf = k0 + fac;
                d2_t x = tj[it];
                if (!(kf > lo && kf < hi)) { x.x = 0.0; x.y = 0.0; }        // factor outside the window: zeros
                *(d2_t*)(LJ + fac * LJS + 2 * pr) = x;
            }
        }
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int e = tid + K3_NT * j;
            if (e < (AT + 3) * BTW_OUT) { const int sl = e / BTW_OUT; LB[sl * LBS + (e - sl * BTW_OUT)] = tb[j]; }
        }
    }
    K3STAMP(2);   // own loads landed, LDS written
    __syncthreads();
    K3STAMP(3);   // everybody's

    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;   // wave-uniform: the keyframe loop and its tests stay scalar
    assemble_tile<K3_KPW>(v, LJ, LB, s_a, w, b, k0, gk0, lo, hi, rlo, rhi, wv, lane, maps);
    K3STAMP(4);       // wave 0: MFMAs done, stores issued
#ifdef VF_SOLVE_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    K3STAMP(5);       // ... and acknowledged
#endif
}
