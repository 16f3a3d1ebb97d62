// kernels/k4_band_body.inc -- K4: the LDS maps and band_solve_body<MODE>, the one body of every block-banded Cholesky sweep (whole window, twisted,
// chunk, split, assembling, two-wave assembling, incremental suffix).
// A section of vf_kernels.hip (ONE translation unit); included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ K4
VF_DI double readlane_d(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// One wavefront per window.  Right-looking block Cholesky of the block-banded normal matrix,
// exploiting its profile: IMU factors couple consecutive keyframes in all 15 dof, between
// factors couple keyframes up to 3 apart in the 6 pose dof only, so the active set while
// eliminating keyframe k is  [k: 15] [k+1: 15] [k+2: pose 6] [k+3: pose 6]  = 42 rows.
// The panel of step k has 58 rows, one per lane:
//     0..14  pivot block          15..41  sub-diagonal rows        42  right-hand side
//    43..57  identity  -> after the column operations these rows hold L_kk^-T
// (the rhs row makes the forward substitution free, the identity rows turn the back substitution
// into a mat-vec instead of a 15-step triangular chain).
//   * panel factorisation in registers, as generated straight-line code in a fixed issue order (tools/gen_pivot.py,
//     vf_pivot_15.inc): the chain pivot c -> c+1 (scale, v_readlane the multiplier, update, v_readlane the next pivot,
//     v_rsq_f64 + one third-order correction) interleaved with the other columns' updates -- the two nearest by
//     v_readlane broadcasts issued one ahead of their use, the rest by one v_fmac_f64_dpp row_newbcast each; a
//     non-positive pivot shows as NaN / inf in the last reciprocal, tested once per step;
//   * Schur update of the trailing 28x27 block (27 active rows + rhs) = C - P P^T on the matrix
//     cores: 3 lower tiles x 4 k-steps of v_mfma_f64_16x16x4, operands straight from the LDS panel, the trailing
//     entries as accumulator input (negated A operands), results written back without a read-out pass;
//   * trailing window: circular 4-keyframe LDS buffer.  The k loop is unrolled by 4 so that the
//     slot arithmetic ((k+d)&3) is a compile-time constant: every LDS address is a per-lane
//     constant plus an immediate; block rows of H are fetched from HBM three steps ahead, unconditionally
//     (absent blocks come from a row of zeros);
//   * panel rows 15..57 go to HBM straight from registers, by column pairs (see "Panel" below);
//   * back substitution software-pipelined: the increment of the previous step stays in registers (v_readlane
//     broadcasts), everything that does not depend on it is prepared one step ahead.
// One-wave workgroup: LDS operations of a wave retire in issue order, so cross-lane hand-offs
// through LDS need no s_barrier and no vmcnt(0) (which __syncthreads() carries and which would
// stall every step on the in-flight HBM prefetch); a compiler barrier (+ lgkmcnt(0) where a value is used) is enough.
// The same holds between the two waves of the two-wave sweep: their hand-shake cells are read with ds_read (lds_peek, lds_ask),
// never through a volatile generic pointer, which compiles to flat_load + s_waitcnt vmcnt(0).  The only vmcnt waits inside a
// step loop are the counted ones the compiler puts in front of the uses of prefetched registers (block rows, J tiles); the last
// word of a J tile is waited for with vmcnt(0), in the one step of eight that puts a tile in place.
// Sequential in k: latency-bound for one window, HBM-bound (5 TB/s) under a full batch; see DESIGN.md "K4".
constexpr int LDW = 61;
// Panel of one keyframe in HBM (vf_kernels.hpp "Cholesky panel"): column pairs, lane = row, so one 16-byte store / load
// instruction of the sweeps covers up to 43 x 16 contiguous bytes -- with a row per 128-B line every instruction touched 43
// different lines, 16 bytes of each.  The offset of a lane's entry of pair c is a per-lane constant (its place in the pair,
// or the keyframe's zero cell where the entry is a structural zero of L^-T): no predicate in either sweep.
// a wave-uniform pointer into global memory, told to the compiler as such (SGPR base + per-lane 32-bit offset addressing)
#define VF_GLOBAL __attribute__((address_space(1)))
template <class T> VF_DI VF_GLOBAL char* uniform_gptr(T* p) {
    const unsigned long long x = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)(x >> 32));
    return (VF_GLOBAL char*)(((unsigned long long)hi << 32) | lo);
}
VF_DI int panel_pair_off(int row, int c) { return (row < panel_rows(c) ? panel_off(c) + 2 * row : PANEL_DUMP) * (int)sizeof(double); }
constexpr int S_WD = 0;                  // LDS map (doubles)
constexpr int S_GD = 60 * LDW;           // 3660: rhs, circular
constexpr int S_DUMP = S_GD + 64;        // write sink for masked-off lanes (never read)
constexpr int S_ZERO = S_DUMP + 96;      // 16 zeros: read source for masked-off lanes
constexpr int S_ID = S_ZERO + 16;        // 15x15 identity: panel rows of the L^-T lanes
constexpr int S_P = S_ID + 225;          // panel rows 15..42 at stride 15 (conflict-free column reads)
constexpr int S_DL = S_P + 43 * 15;      // back-substitution: delta of the 3 following keyframes
constexpr int S_BC = S_DL + 64;          // 16: pivot-block entries of the column just scaled, read back replicated per 16-lane row
constexpr int S_TOTAL = S_BC + 16;
// Compact trailing window of the SPLIT forward sweep (SOLVE_FULL_FWD, k_band_forward): 20.2 KB of LDS per wave instead of 38.3,
// i.e. EIGHT one-wave workgroups per CU = two resident waves per SIMD (the kernel's 252 registers allow that too).
// The 60 x 61 window above keeps every (row slot, column slot) pair of its four circular keyframe slots, although only
// the lower block triangle within the profile [k: 15][k+1: 15][k+2: pose][k+3: pose] is ever live.  Here a block is filed
// under the slot of its ROW keyframe and its DISTANCE e to the column keyframe -- both stay the same while the sweep
// moves on (row and column keyframe age together), so nothing is ever copied or promoted:
//     e = 0: lower triangle, 120      e = 1: 15 x 15      e = 2: 6 x 15 (pose rows; fill-in and the marginal prior's strip)
//     e = 3: 6 x 6 (pose x pose; a panel row of that block is read 15 wide and its columns 6..14 are masked to zero)
// the identity rows of the panel come from a 29-cell strip (0 x 14, 1, 0 x 14) read at a per-lane offset.
constexpr int CW_D0 = 0, CW_D1 = 120, CW_D2 = CW_D1 + 225, CW_D3 = CW_D2 + 90, CW_SLOT = CW_D3 + 36;
constexpr int CW_GD = 4 * CW_SLOT;           // rhs, circular (4 x 15, padded to 64)
constexpr int CW_DUMP = CW_GD + 64;
constexpr int CW_ZERO = CW_DUMP + 96;
constexpr int CW_ID = CW_ZERO + 16;          // identity strip: cell 14 = 1
constexpr int CW_P = CW_ID + 30;             // panel rows 15..42 at stride 15 (MFMA operands)
constexpr int CW_BC = CW_P + 28 * 15;
constexpr int CW_TOTAL = CW_BC + 16;
static_assert(CW_TOTAL * 8 <= 20480, "eight compact forward sweeps per CU (160 KB of LDS)");
// Assembling forward sweep (SOLVE_ASM_FWD, k_band_forward_asm): the compact window, then the LDS image of ONE tile of the J
// stream (8 factors at K3's stride LJS: pairs, residual, zero cell) and ONE between linearisation (78 words + the zero cell).
constexpr int AS_LJ = CW_TOTAL, AS_LB = AS_LJ + JT * LJS, AS_TOTAL = AS_LB + 80;
constexpr int AS_FLAGS = AS_TOTAL, AS2_TOTAL = AS_FLAGS + 8;     // two-wave form: [0] steps begun by the eliminator, [1] rows committed by the assembler, [2] J tiles put in place by the eliminator
static_assert(AS_LJ % 2 == 0 && AS2_TOTAL * 8 <= 40960, "four assembling sweeps per CU (one per SIMD)");
// chunk forward sweep with a spike follower (k_chunk_forward): the panel of step k (43 rows x 15, then a
// zero cell and a write sink) stays in a 4-slot LDS ring for the second wave; two hand-shake cells follow
constexpr int RING_SLOT = 664;
constexpr int S_PROG = S_P + 4 * RING_SLOT;   // panels completed by the sweep
constexpr int S_CONS = S_PROG + 1;            // panels consumed by the follower
constexpr int S_RING_OUT = S_PROG + 2;        // != 0: a wait on the ring ran out (the chunk's solve is reported failed; later waits do not wait)
constexpr int RING_SPIN_MAX = 1 << 22;        // polls (each an LDS read + s_sleep): seconds, against the microseconds a step takes
constexpr int S_BC_RING = S_PROG + 8;
constexpr int S_TOTAL_RING = S_BC_RING + 16;
#ifndef VF_ASM2_ROLES
#define VF_ASM2_ROLES 1     // two-wave assembling sweep: 1 = the workgroups of a CU agree on one eliminator per SIMD (View::place), 2 = wave 1 eliminates in every workgroup (test build)
#endif
static_assert(VF_ASM2_ROLES == 1 || VF_ASM2_ROLES == 2, "the roles of the two-wave assembling sweep are agreed per CU (1) or swapped in every workgroup (2, test build)");
#define WSYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define VF_PIVOT_SLOT(i) do {} while (0)     // places the generated pivot code leaves for its caller (tools/gen_pivot.py)
constexpr int ASM2_CHUNK = 1024;    // windows per launch of the two-wave assembling sweep
#define VF_SB() __builtin_amdgcn_sched_barrier(0)
#ifdef VF_SOLVE_STAMPS   // diagnostic build only (tools/build_stamps.sh); never in the shipped library
__device__ unsigned long long g_stamps[16];
#define STAMP(i) do { __builtin_amdgcn_sched_barrier(0); unsigned long long _t; asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t) :: "memory"); __builtin_amdgcn_sched_barrier(0); if (w == 0) st[i] += _t - tprev; tprev = _t; } while (0)
#else
#define STAMP(i) do {} while (0)
#endif
// uncached read of an LDS cell another wave of the workgroup writes (hand-shake counters)
VF_DI double lds_peek(const double* p) {
    double x;
    const unsigned addr = (unsigned)(size_t)p;    // low half of a flat LDS address = LDS offset
    asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(x) : "v"(addr) : "memory");
    return x;
}
// the same read issued and NOT waited for, for a value that is wanted later: a relaxed workgroup-scope atomic load through an
// LDS-address-space pointer, i.e. one ds_read_b64 the compiler counts in lgkmcnt itself and waits for in front of the first use.
// (Never a volatile access through the generic pointer: that stays a flat_load with sc0 sc1 and gets s_waitcnt vmcnt(0)
// behind it -- a drain of every panel store and tile load in flight, once per step: NOTEBOOK.md 7.17.)
#define VF_LDS __attribute__((address_space(3)))
VF_DI double lds_ask(const double* p) {
    const VF_LDS long long* q = (const VF_LDS long long*)(size_t)(unsigned)(size_t)p;    // low half of a flat LDS address = LDS offset
    return __longlong_as_double(__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}

// TW = false: one wave sweeps the whole window (throughput form, one window per SIMD).
// TW = true : burn-at-both-ends (twisted) factorisation for one-window latency: wave 0 eliminates
//   keyframes 0 .. t-1 forwards, wave 1 eliminates n-1 .. t+3 backwards (the same code on the
//   reversed sequence: block d of reversed row j is H[j+d][d]^T), they meet at a dense 45x45 system
//   for keyframes t, t+1, t+2, and the two back substitutions run concurrently.  No extra flops.
constexpr int MID_LD = 47;                      // 45 columns + rhs + pad
constexpr int MID_TOTAL = 45 * MID_LD + 48;     // + the 45 solved increments handed to both waves
// MODE 2 / 3 (partitioned solve, K4p): the forward / backward sweep of ONE chunk of a window.  The
//   forward sweep eliminates the chunk's `ni` interior keyframes and leaves the partially reduced
//   45x45 block (+ rhs) of the 3 separator keyframes that follow in `sep_out`; couplings to
//   keyframes in front of the chunk (the left separator) are dropped here and carried by the spike
//   kernel.  The backward sweep starts from the separator increments already in v.delta.
// MODE 4 / 5 (split sweep, batches of >= View::split_min windows): the forward sweep and the back substitution of SOLVE_FULL
//   as two kernels.  They hand over through HBM only (the panels and the rhs row the forward sweep stores anyway); the
//   back substitution needs 9 KB of LDS instead of 38 and so runs two and more waves per SIMD where the fused kernel
//   is held to one by the forward sweep's trailing window.
// MODE 11 (k_band_backward_1w): MODE 5 for batches of at most one window per SIMD (SolvePlan::bwd_one_wave) -- the software-pipelined
//   recursion of SOLVE_FULL's back substitution, four panels in flight, as a kernel held to one wave per SIMD.
// MODE 6 (assembling forward sweep, where solve_plan() picks it: vf_solve_plan.hpp): SOLVE_FULL_FWD that forms the block rows of H itself,
//   from the J stream and the between linearisations K1 / K2 leave, on the matrix cores, under the waits of the pivot
//   chain -- K3 is not launched, H is neither written nor read.  See "assembling sweep" below.
// MODE 7 / 8 (k_band_forward_asm2): MODE 6 as TWO waves of one workgroup sharing its LDS -- wave 0 eliminates (SOLVE_ASM_A: the
//   forward sweep of MODE 4 whose rows somebody else commits), wave 1 assembles (SOLVE_ASM_B: the row recurrence of MODE 6 and
//   nothing else) and writes row k + 4 into the window between the eliminator's read of pivot row k and its Schur update's
//   accumulator reads; two cells of LDS carry the hand-shake.  Eight waves per CU on the LDS of four sweeps: the matrix
//   instructions of the two roles overlap each other's waits, which one wave cannot do for itself (DESIGN.md 7.13, 7.15).
// MODE 9 / 10 (incremental updates, View::inc_*): the forward sweep of SOLVE_FULL started at keyframe cg.i0 of the window from a
//   checkpoint of its trailing window (and leaving one at every CK-th keyframe slot it passes), and the back substitution of
//   SOLVE_FULL_BWD that stops once it reproduces the increments that are there, below keyframe cg.ni of the window.
enum { SOLVE_FULL = 0, SOLVE_TWISTED = 1, SOLVE_CHUNK_FWD = 2, SOLVE_CHUNK_BWD = 3, SOLVE_FULL_FWD = 4, SOLVE_FULL_BWD = 5, SOLVE_ASM_FWD = 6,
       SOLVE_ASM_A = 7, SOLVE_ASM_B = 8, SOLVE_INC_FWD = 9, SOLVE_INC_BWD = 10, SOLVE_FULL_BWD1 = 11 };
template <int MODE>
__device__ __forceinline__ void band_solve_body(const View& v, double* __restrict__ S, double* __restrict__ S_other,
                                                double* __restrict__ MID, const int w, const int lane, const int wave,
                                                const ChunkGeom cg = ChunkGeom{0, 0, 0}, double* __restrict__ sep_out = nullptr) {
    constexpr bool TW = MODE == SOLVE_TWISTED;
    constexpr bool CH = MODE == SOLVE_CHUNK_FWD || MODE == SOLVE_CHUNK_BWD;
    constexpr bool ASA = MODE == SOLVE_ASM_A, ASB = MODE == SOLVE_ASM_B;   // the two roles of the two-wave assembling sweep
    constexpr bool AS = MODE == SOLVE_ASM_FWD || ASB;    // rows of H assembled here (no K3)
    constexpr bool CW = MODE == SOLVE_FULL_FWD || AS || ASA;   // compact trailing window ("CW_" map above); the names below shadow the full map
    constexpr bool INCF = MODE == SOLVE_INC_FWD, INCB = MODE == SOLVE_INC_BWD;
    constexpr bool BWD = MODE == SOLVE_FULL_BWD || MODE == SOLVE_FULL_BWD1;     // the split back substitution, either form
    constexpr int S_GD = CW ? CW_GD : vf::S_GD, S_DUMP = CW ? CW_DUMP : vf::S_DUMP, S_ZERO = CW ? CW_ZERO : vf::S_ZERO;
    constexpr int S_ID = CW ? CW_ID : vf::S_ID, S_P = CW ? CW_P : vf::S_P, S_BC = CW ? CW_BC : vf::S_BC;
    const int lo = v.lo[w], hi = v.hi[w];
    const int n = CH ? cg.ni + (cg.has_sep ? 3 : 0) : hi - lo - (INCF ? cg.i0 : 0);     // real rows of this sweep
    const double lam = v.lambda[w];
    const size_t base = (size_t)w * v.M + lo + ((CH || INCF) ? cg.i0 : 0);
    int failed = 0;
    // sweep geometry: sweep index kk -> window keyframe j(kk); kinds of rows: 0 real, 1 identity, 2 zero
    const bool rev = TW && wave == 1;
    const int tsp = TW ? (((n - 3) / 2) & ~3) : 0;                 // split keyframe (multiple of 4)
    const int cr = TW ? n - tsp - 3 : 0;                            // pivots of the reverse sweep
    const int qpad = TW ? ((4 - (cr & 3)) & 3) : 0;                 // identity pads in front of it
    const int npiv = CH ? cg.ni : n;                                // real pivots of a one-directional sweep
    const int cnt = !TW ? ((CH && cg.has_sep) ? cg.ni : ((npiv + 3) & ~3))
                        : (rev ? cr + qpad : tsp);                  // pivots of this sweep (multiple of 4)
    auto row_kind = [=](int kk) {
        if (!TW) return kk < n ? 0 : 1;
        if (!rev) return kk < tsp + 3 ? 0 : 1;
        if (kk < qpad) return 1;
        const int j = n - 1 - (kk - qpad);
        return j >= tsp + 3 ? 0 : (j >= tsp ? 2 : 1);
    };
    auto kf_of = [=](int kk) { return rev ? n - 1 - (kk - qpad) : kk; };   // window-local keyframe of a real row
    auto pivot_real = [=](int kk) { return !TW ? kk < npiv : (rev ? kk >= qpad : true); };

    // ---- per-lane constants.  Every LDS access below is branch-free: masked-off lanes read the
    // zero cells / write the sink, so no exec-mask juggling (and no SGPR spills) in the k loop.
    if constexpr (CW) { if (lane < 46) S[S_ZERO + lane] = lane == 16 + 14 ? 1.0 : 0.0; }     // 16 zeros, then the identity strip
    else for (int e = lane; e < 16 + 225; e += 64) S[S_ZERO + e] = (e >= 16 && (e - 16) % 16 == 0) ? 1.0 : 0.0;
    const int pd = lane < 15 ? 0 : (lane < 30 ? 1 : (lane < 36 ? 2 : 3));
    const int pa = lane < 15 ? lane : (lane < 30 ? lane - 15 : (lane < 36 ? lane - 30 : lane - 36));
    int ri_ph[4];   // LDS offset of (this lane's panel row, column 0 of the pivot slot) per phase
#pragma unroll
    for (int ph = 0; ph < 4; ph++) {
        const int s0 = ph * 15;
        if constexpr (CW) {
            const int blk = pd == 0 ? CW_D0 + h_tri(pa, 0) : (pd == 1 ? CW_D1 + pa * 15 : (pd == 2 ? CW_D2 + pa * 15 : CW_D3 + pa * 6));
            ri_ph[ph] = lane < 42 ? ((ph + pd) & 3) * CW_SLOT + blk
                      : (lane == 42 ? S_GD + s0 : (lane < 58 ? S_ID + 14 - (lane - 43) : S_ZERO));
        } else
        ri_ph[ph] = lane < 42 ? S_WD + ((((ph + pd) & 3) * 15) + pa) * LDW + s0
                  : (lane == 42 ? S_GD + s0 : (lane < 58 ? S_ID + (lane - 43) * 15 : S_ZERO));
    }
    // lanes 58..63 read 15 consecutive cells from S_ZERO: S_ZERO has 16 zeros -> a zero row
    constexpr bool RINGM = MODE == SOLVE_CHUNK_FWD;        // panels also feed the spike follower (LDS ring)
    constexpr int RSLOT = RINGM ? RING_SLOT : 0;
    const int pw_off = (lane >= 15 && lane < (RINGM ? 58 : 43)) ? S_P + (lane - 15) * 15
                                                                : (RINGM ? S_P + 646 : S_DUMP + 16);   // sub-panel -> LDS
    // (the ring's zero cells and hand-shake counters are initialised by k_chunk_forward BEFORE the two waves part:
    // the follower must never poll a counter left over in LDS by an earlier workgroup)
    const int op_zero = RINGM ? S_P + 645 : S_ZERO;
    const bool follower = RINGM && cg.i0 > 0;              // chunk 0 has no left separator, hence no spike
    // Schur write-back targets (MFMA C layout): tile t in {(0,0),(1,0),(1,1)}, register r:
    //   i = 16*Ti + (lane>>4) + 4r (trailing row, 27 = rhs), j = 16*Tj + (lane&15)
    int tgt_ph[4][12];
    // (the eliminator wave of the two-wave assembling sweep has 256 registers and keeps a J tile in 80 of them: it holds one
    // base per target and forms the four phases' addresses as base + step * ((phase + shift) & 3) when it uses them)
    int tgB[12] = {}, tgM[12] = {};
#pragma unroll
    for (int q = 0; q < 12; q++) {
        const int t = q >> 2, r = q & 3;
        const int Ti = t == 0 ? 0 : 1, Tj = t == 2 ? 1 : 0;
        const int i = 16 * Ti + (lane >> 4) + 4 * r, j = 16 * Tj + (lane & 15);
        const int rs = i < 15 ? 1 : (i < 21 ? 2 : 3), ra = i < 15 ? i : (i < 21 ? i - 15 : i - 21);
        const int cs = j < 15 ? 1 : (j < 21 ? 2 : 3), ca = j < 15 ? j : (j < 21 ? j - 15 : j - 21);
        const bool valid = i <= 27 && j <= 26 && j <= i;
#pragma unroll
        for (int ph = 0; ph < 4; ph++) {
            const int cj = (((ph + cs) & 3) * 15) + ca;
            if constexpr (CW) {
                const int e = rs - cs;   // 0, 1, 2 (rows k+1 .. k+3 against columns k+1 .. k+3)
                const int blk = e == 0 ? CW_D0 + h_tri(ra, ca) : (e == 1 ? CW_D1 + ra * 15 + ca : CW_D2 + ra * 15 + ca);
                if constexpr (ASA) {
                    tgB[q] = !valid ? S_DUMP + 32 + lane : (i == 27 ? S_GD + ca : blk);
                    tgM[q] = !valid ? 0 : (i == 27 ? 15 | (cs << 16) : CW_SLOT | (rs << 16));
                } else
                tgt_ph[ph][q] = !valid ? S_DUMP + 32 + lane : (i == 27 ? S_GD + cj : ((ph + rs) & 3) * CW_SLOT + blk);
            } else
            tgt_ph[ph][q] = !valid ? S_DUMP + 32 + lane
                                   : (i == 27 ? S_GD + cj : S_WD + ((((ph + rs) & 3) * 15) + ra) * LDW + cj);
        }
    }
    // MFMA operands: P[15 + 16*T + (lane&15)][4*q + (lane>>4)]; outside the 28x15 panel -> zero cell
    int op0[4], op1[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int kc = 4 * q + (lane >> 4);
        op0[q] = kc < 15 ? S_P + (lane & 15) * 15 + kc : op_zero;
        op1[q] = (kc < 15 && 31 + (lane & 15) <= 42) ? S_P + (16 + (lane & 15)) * 15 + kc : op_zero;
    }
    // block-row commit maps (vf_kernels.hpp "Block row of H"): per lane, where the words it loads go in a slot of the window
    //   d1: idx = lane + 64 j over the 15x15 block -> (a, c)
    int cm_off[4], cm_srcT[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int idx = lane + 64 * j, a = idx / 15, c = idx - a * 15;
        const bool in = idx < 225;
        cm_off[j] = in ? a * LDW + c : -1;
        cm_srcT[j] = in ? c * 15 + a : 0;            // transposed read for the reverse sweep
    }
    //   d0: e = lane + 64 j over the 120 entries of the lower triangle -> (a, c <= a); the diagonal gets +lambda
    int t0_off[2], t0_a[2], t0_c[2];
    double t0_lam[2], t0_one[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int e = lane + 64 * j;
        int a = 0;
        while (h_tri(a + 1, 0) <= e && a < 14) a++;
        const int c = e - h_tri(a, 0);
        const bool in = e < 120;
        t0_a[j] = in ? a : -1;
        t0_c[j] = in ? c : -2;
        t0_off[j] = in ? a * LDW + c : -1;
        t0_lam[j] = (in && a == c) ? lam : 0.0;
        t0_one[j] = (in && a == c) ? 1.0 : 0.0;
    }
    //   d2, d3: 6x6 pose x pose (lane < 36); dx: 6x9 (pose) x (velocity / bias), columns 6..14 (lane < 54)
    const int s6_off = lane < 36 ? (lane / 6) * LDW + lane % 6 : -1;
    const int s6_srcT = lane < 36 ? (lane % 6) * 6 + lane / 6 : 0;      // reverse sweep: transposed
    const int x9_off = lane < 54 ? (lane / 9) * LDW + 6 + lane % 9 : -1;
    const double mp_third = (v.mp_on[w] && n >= 3 && !rev && ((!CH && !INCF) || cg.i0 == 0)) ? 1.0 : 0.0;
    WSYNC();

    // ---- assembling sweep (AS): the block row of keyframe R is formed here instead of being read from H --------------------
    // One "iteration" per row, K3's recurrence on one wave: with the operands of IMU factor R+1 in LDS (i side = keyframe R,
    // j side = keyframe R+1; column 15 of an operand tile carries the whitened residual, so J^T r comes with J^T J)
    //     Dfin = D + Ji^T [Ji | r]                       diagonal block + gradient of row R        (D: started one iteration ago)
    //     On   = Jj^T Ji,  Dn = Jj^T [Jj | r]            coupling block and start of the diagonal of row R+1
    //     Z    = X^T X,  X = [Ja | Jb | 0 0 0 | r]       everything the between factor ending at R contributes, in ONE tile (6 rows =
    //                                                    two k-steps): Z[0:6, 0:6 | 15] = Ja^T [Ja | r] goes to the diagonal block +
    //                                                    gradient of row R - d (still in the window), Z[6:12, 6:12 | 15] = Jb^T [Jb | r]
    //                                                    to those of row R, Z[6:12, 0:6] = Jb^T Ja is the pose block of row R against R - d
    // 14 v_mfma_f64_16x16x4 per row (a single wave gets one through every ~125 cycles, so their number is the price of the
    // fusion: with the three between products formed separately there were 18); inside the elimination loop they are issued one at a time from the places the generated
    // pivot code leaves for them (VF_PIVOT_SLOT), i.e. under the waits of the chain.  The J stream is read as K3 reads it --
    // whole tiles of 8 factors, every 128-B line once -- but one tile per 8 steps: the next tile waits in registers (19
    // 16-byte words per lane) and is written to LDS when the last factor of the current one has been used.  A between
    // factor's term on its OLDER keyframe goes into that row's slot of the window (the row is at most three steps from its
    // elimination, so it is still there), which is why one staged between linearisation is enough.
    struct Asm { d4_t D, O, Dfin, Z, On, Dn; double ai[4], aj[4], xx[2]; int d, d_next; };
    struct AsmNext { d2_t tj[19]; double tr[2], blA[2], blB[2]; int aA, aB, k0_next, tiles_wanted; };
    constexpr int AS_NOWN = JS_PAIRS * JT;                       // 16-byte words of a tile
    const int as_b = (AS || ASA) ? v.sel[w] : 0;
    AsmMaps am = {};
    int as_cD[4] = {}, as_cDs[4] = {}, as_cO[4] = {}, as_c1[2] = {}, as_c2[2] = {}, as_c3[2] = {}, as_rB[2] = {}, as_rS[2] = {}, as_bB[2] = {}, as_bS[2] = {}, as_oX[2] = {};
    // (signs and the diagonal's lambda are lane properties, formed where used: the window keeps -g, and the gradient is column 15 of every tile)
    const double as_sgn = (lane & 15) == 15 ? -1.0 : 1.0;
    const int as_hx = lane < 54 ? CW_D2 + (lane / 9) * 15 + 6 + lane % 9 : -1;
    if constexpr (AS) {
        am = make_asm_maps(v, w, lo, hi, lane);
        const int ci = lane & 15, kq = lane >> 4;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int a = kq + 4 * r;
            const bool tri = a < 15 && ci <= a, grad = a < 15 && ci == 15;
            as_cD[r] = tri ? CW_D0 + h_tri(a, ci) : (grad ? S_GD + a : S_DUMP + 32 + lane);      // + PH * as_cDs
            as_cDs[r] = tri ? CW_SLOT : (grad ? 15 : 0);
            as_cO[r] = (a < 15 && ci < 15) ? CW_D1 + a * 15 + ci : -1;
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            // rows 0..5 of Z (registers 0, 1): the older keyframe's term, into that row's slot
            const int a6 = kq + 4 * r;
            const bool tri = a6 < 6 && ci <= a6, grad = a6 < 6 && ci == 15;
            as_rB[r] = tri ? CW_D0 + h_tri(a6, ci) : (grad ? S_GD + a6 : S_DUMP + 32 + lane);   // + slot * as_rS
            as_rS[r] = tri ? CW_SLOT : (grad ? 15 : 0);
            // rows 6..11 of Z (registers 1, 2): columns 0..5 = the pose block against R - d, columns 6..11 | 15 = this row's own term
            const int b6 = kq + 4 * (r + 1) - 6;
            const bool brow = b6 >= 0 && b6 < 6;
            const bool in = brow && ci < 6;
            as_c1[r] = in ? CW_D1 + b6 * 15 + ci : -1;
            as_c2[r] = in ? CW_D2 + b6 * 15 + ci : -1;
            as_c3[r] = in ? CW_D3 + b6 * 6 + ci : -1;
            const bool btri = brow && ci >= 6 && ci - 6 <= b6, bgrad = brow && ci == 15;
            as_bB[r] = btri ? CW_D0 + h_tri(b6, ci - 6) : (bgrad ? S_GD + b6 : S_DUMP + 32 + lane);   // + PH * as_bS
            as_bS[r] = btri ? CW_SLOT : (bgrad ? 15 : 0);
            // operand word of k-step r: X[4 r + kq][ci] in the staged linearisation (r: 0, Ja: 6, Jb: 42; its pad cell is zero)
            const int row = 4 * r + kq;
            as_oX[r] = row >= 6 ? BTW_OUT : (ci < 6 ? 6 + row * 6 + ci : (ci < 12 ? 42 + row * 6 + ci - 6 : (ci == 15 ? row : BTW_OUT)));
        }
        if (lane < JT) S[AS_LJ + lane * LJS + LJ_ZERO] = 0.0;
        if (lane < 2) S[AS_LB + BTW_OUT + lane] = 0.0;
    }
    const size_t as_tiles = (size_t)(v.G >> 6);
    // loads of the J tile that holds window slot k0 (a multiple of 8) and of its 8 residual vectors
    auto as_tile_fetch = [=](int k0, AsmNext& nx) {
        long gt = ((long)w * v.M + k0) >> JT_LOG;
        const long gmax = (v.G >> JT_LOG) - 1;
        gt = gt > gmax ? gmax : gt;                          // (rows past the window's end: any tile, zeroed at commit)
        const d2_t* jt = (const d2_t*)(v.imu_j + ((size_t)as_b * (size_t)(v.G >> JT_LOG) + (size_t)gt) * JT_STRIDE);
#pragma unroll
        for (int it = 0; it < 19; it++) {
            const int e = it * 64 + lane;
            nx.tj[it] = jt[e < AS_NOWN ? e : AS_NOWN - 1];
        }
        const double* rb = v.imu_r + (size_t)as_b * as_tiles * IMU_R * TILE;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int e = lane + 64 * j < JT * IMU_R ? lane + 64 * j : JT * IMU_R - 1;
            const int fac = e / IMU_R, a = e - fac * IMU_R;
            const long gf = (gt << JT_LOG) + fac;
            nx.tr[j] = rb[((size_t)(gf >> 6) * IMU_R + a) * TILE + (gf & 63)];
        }
    };
    auto as_tile_commit = [&](int k0, const AsmNext& nx) {
        // word e = 64 it + lane of the tile is pair 8 it + (lane >> 3) of factor lane & 7: one address per lane, the rest immediates
        const int fac = lane & (JT - 1), kf = k0 + fac;
        const bool keep = kf > lo && kf < hi;                    // a factor outside the window contributes zeros
        double* dst = S + AS_LJ + fac * LJS + 2 * (lane >> JT_LOG);
#pragma unroll
        for (int it = 0; it < 19; it++) {
            d2_t x = nx.tj[it];
            x.x = keep ? x.x : 0.0;
            x.y = keep ? x.y : 0.0;
            if (it < 18 || lane < AS_NOWN - 18 * 64) *(d2_t*)(dst + it * (2 * 64 / JT)) = x;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int e = lane + 64 * j;
            const int f2 = e / IMU_R, a = e - f2 * IMU_R, kf2 = k0 + f2;
            if (e < JT * IMU_R) S[AS_LJ + f2 * LJS + LJ_R + a] = (kf2 > lo && kf2 < hi) ? nx.tr[j] : 0.0;
        }
    };
    // between linearisation of the factor ending at sweep row R (words lane, lane + 64 of 78) and its older keyframe (-1: none)
    // (the older keyframe comes back as loaded, one copy per lane: decoding it here would wait for the load on the spot)
    auto as_btw_fetch = [=](int R, double (&bl)[2], int& a_raw) {
        const int ks = lo + R;
        long gs = (long)w * v.M + ks;
        gs = gs < v.G ? gs : v.G - 1;
        a_raw = v.btw_a[gs];
        const double* bo = v.btw_out + (size_t)as_b * as_tiles * BTW_OUT * TILE + (size_t)(gs >> 6) * BTW_OUT * TILE + (gs & 63);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int f = lane + 64 * j < BTW_OUT ? lane + 64 * j : BTW_OUT - 1;
            bl[j] = bo[(size_t)f * TILE];
        }
    };
    // distance 1..3 from row R to the older keyframe of the between factor ending there; 0 = no factor
    auto as_btw_dist = [=](int R, int a_raw) {
        const int ks = lo + R;
        const int a = __builtin_amdgcn_readfirstlane(a_raw);
        return (R > 0 && ks < hi && a >= lo && a < ks) ? ks - a : 0;
    };
    auto as_btw_commit = [&](const double (&bl)[2], int d) {
        S[AS_LB + lane] = d > 0 ? bl[0] : 0.0;
        S[lane + 64 < BTW_OUT ? AS_LB + lane + 64 : S_DUMP + 32 + lane] = d > 0 ? bl[1] : 0.0;
    };
    // the matrix-core work of one iteration, cut into the pieces the pivot code's places take (piece 0: operand reads)
    auto as_piece = [&](auto i_, Asm& z, const int fimg) {
        constexpr int I = decltype(i_)::value;
        auto mf = [](double a, double b, d4_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); };
        if constexpr (I == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) { z.ai[q] = S[fimg + am.offI[q]]; z.aj[q] = S[fimg + am.offJ[q]]; }
#pragma unroll
            for (int q = 0; q < 2; q++) z.xx[q] = S[AS_LB + as_oX[q]];
        }
        else if constexpr (I == 2) z.Dfin = mf(z.ai[0], z.ai[0], z.D);
        else if constexpr (I == 3) z.Dn = mf(z.aj[0], z.aj[0], (d4_t){0, 0, 0, 0});
        else if constexpr (I == 4) z.On = mf(z.aj[0], z.ai[0], (d4_t){0, 0, 0, 0});
        else if constexpr (I == 5) z.Z = mf(z.xx[0], z.xx[0], (d4_t){0, 0, 0, 0});
        else if constexpr (I == 7) z.Dfin = mf(z.ai[1], z.ai[1], z.Dfin);
        else if constexpr (I == 8) z.Dn = mf(z.aj[1], z.aj[1], z.Dn);
        else if constexpr (I == 9) z.On = mf(z.aj[1], z.ai[1], z.On);
        else if constexpr (I == 10) z.Z = mf(z.xx[1], z.xx[1], z.Z);
        else if constexpr (I == 12) z.Dfin = mf(z.ai[2], z.ai[2], z.Dfin);
        else if constexpr (I == 13) z.Dn = mf(z.aj[2], z.aj[2], z.Dn);
        else if constexpr (I == 14) z.On = mf(z.aj[2], z.ai[2], z.On);
        else if constexpr (I == 15) z.Dfin = mf(z.ai[3], z.ai[3], z.Dfin);
        else if constexpr (I == 16) z.Dn = mf(z.aj[3], z.aj[3], z.Dn);
        else if constexpr (I == 17) z.On = mf(z.aj[3], z.ai[3], z.On);
    };
    // A into the diagonal block / gradient of row R - d, which sits in slot (PH - d) & 3 of the window.  Issued after the
    // write-back of the previous step's Schur update and before this step's reads of it (LDS operations of a wave retire in order).
    auto as_rmw = [&](auto ph, const Asm& z) {
        constexpr int PH = decltype(ph)::value;
        if (z.d > 0) {
            const int sa = (PH + 4 - z.d) & 3;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const int addr = as_rB[r] + sa * as_rS[r];
                S[addr] = fma(as_sgn, z.Z[r], S[addr]);
            }
        }
    };
    // row R (sweep index, R & 3 == PH) into the slot the pivot keyframe frees
    // (SPECIAL: the rows that can carry the prior / the marginal prior -- the first four, committed in front of the loop; a
    // prior on a later keyframe is added by as_late_prior.  Their code, 150 loads, stays out of the elimination loop.)
    auto as_commit = [&](auto ph, auto special_, int R, const Asm& z) {
        constexpr int PH = decltype(ph)::value;
        constexpr bool SPECIAL = decltype(special_)::value != 0;
        constexpr int sb = PH * CW_SLOT;
        const int ci = lane & 15, kq = lane >> 4;
        const int kind = row_kind(R);
        const double dg = kind == 0 ? lam : (kind == 1 ? 1.0 : 0.0);
        d4_t Dv = z.Dfin, Ov = z.O;
        double t2[2], t3[2], hxv = 0.0;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            t2[r] = z.d == 2 ? z.Z[r + 1] : 0.0;        // (rows 6..11 of Z)
            t3[r] = z.d == 3 ? z.Z[r + 1] : 0.0;
        }
        const int k = lo + R;
        const bool is_prior = SPECIAL && am.prior_key == k && kind == 0;
        const int mo = (SPECIAL && am.marg_on && kind == 0) ? R : 99;
        if (SPECIAL && (is_prior || mo < 3)) {       // (wave-uniform, the window's first rows only) the prior and the marginal prior, as K3 adds them
            const double* Pq = v.prior_out + ((size_t)as_b * v.B + w) * PRIOR_OUT;
            const double* ML = v.mp_L + (size_t)w * 729;
            const double* Mg = v.mp_out + ((size_t)as_b * v.B + w) * 28;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int a = kq + 4 * r;
                double add = 0.0;
                if (is_prior && a < 15) {
                    double sum = 0.0;
                    for (int rr = 0; rr < 15; rr++)
                        sum = fma(Pq[15 + rr * 15 + a], ci < 15 ? Pq[15 + rr * 15 + ci] : Pq[rr], sum);
                    add += sum;
                }
                if (mo == 0 && a < 15) add += ci < 15 ? ML[a * 27 + ci] : Mg[a];
                if ((mo == 1 || mo == 2) && a < 6 && (ci < 6 || ci == 15)) {
                    const int ob = mo == 1 ? 15 : 21;
                    add += ci < 6 ? ML[(ob + a) * 27 + ob + ci] : Mg[ob + a];
                }
                Dv[r] += add;
                if (mo == 1 && a < 6 && ci < 15) Ov[r] += ML[(15 + a) * 27 + ci];                 // (lo+1 pose) x (lo: 15)
                if (mo == 2 && a < 6 && ci < 6) Ov[r] += ML[(21 + a) * 27 + 15 + ci];             // (lo+2 pose) x (lo+1 pose)
            }
            if (mo == 2) {
#pragma unroll
                for (int r = 0; r < 2; r++) { const int b6 = kq + 4 * (r + 1) - 6; if (b6 >= 0 && b6 < 6 && ci < 6) t2[r] += ML[(21 + b6) * 27 + ci]; }
                if (lane < 54) hxv = ML[(21 + lane / 9) * 27 + 6 + lane % 9];                       // (lo+2 pose) x (velocity / bias of lo)
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) S[as_cD[r] + PH * as_cDs[r]] = fma(as_sgn, Dv[r], (lane & 15) == (lane >> 4) + 4 * r ? dg : 0.0);
#pragma unroll
        for (int r = 0; r < 4; r++) S[as_cO[r] >= 0 ? sb + as_cO[r] : S_DUMP + 32 + lane] = Ov[r];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            S[as_c2[r] >= 0 ? sb + as_c2[r] : S_DUMP + 32 + lane] = t2[r];
            S[as_c3[r] >= 0 ? sb + as_c3[r] : S_DUMP + 32 + lane] = t3[r];
        }
        S[as_hx >= 0 ? sb + as_hx : S_DUMP + 32 + lane] = hxv;
        // the between factor's own-row term, and its pose block when it reaches back one keyframe only (that block is part of
        // the 15 x 15 coupling written above): read-modify-write behind the stores (LDS operations retire in order)
        if (z.d > 0) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const int addr = as_bB[r] + PH * as_bS[r];
                S[addr] = fma(as_sgn, z.Z[r + 1], S[addr]);
            }
            if (z.d == 1) {
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    const int addr = as_c1[r] >= 0 ? sb + as_c1[r] : S_DUMP + 32 + lane;
                    S[addr] = S[addr] + z.Z[r + 1];
                }
            }
        }
    };
    // a prior on a keyframe beyond the first four rows: J^T [J | r] is formed in front of the loop (as_lp: this lane's four
    // words of the tile), and added to the row when it has just been committed (slot R & 3), before any step reads it
    double as_lp[4] = {0.0, 0.0, 0.0, 0.0};
    const int as_lp_row = (AS && am.prior_key >= lo + 4 && am.prior_key < hi) ? am.prior_key - lo : -1;
    if constexpr (AS) {
        if (as_lp_row >= 0) {
            const int ci = lane & 15, kq = lane >> 4;
            const double* Pq = v.prior_out + ((size_t)as_b * v.B + w) * PRIOR_OUT;
#pragma unroll 1
            for (int rr = 0; rr < 15; rr++) {
                const double cv = ci < 15 ? Pq[15 + rr * 15 + ci] : Pq[rr];
#pragma unroll
                for (int r = 0; r < 4; r++) { const int a = kq + 4 * r; as_lp[r] = fma(a < 15 ? Pq[15 + rr * 15 + a] : 0.0, cv, as_lp[r]); }
            }
        }
    }
    auto as_late_prior = [&](int R) {
        if (R == as_lp_row) {
            const int sl = R & 3;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int addr = as_cD[r] + sl * as_cDs[r];
                S[addr] = fma(as_sgn, as_lp[r], S[addr]);
            }
        }
    };
    // Once the operands of iteration R are in registers (piece 0), the between linearisation of row R+1 may take their place
    // in LDS: its loads are two steps old, and the newest stores in front of them in the memory queue -- the panel of
    // the previous step -- a whole step, so the wait this needs is short (at the end of the step it would stand behind
    // the panel stores just issued: 2 300 cycles per step, measured).  The loads of row R+3 go out behind it.
    auto as_stage_btw = [&](int R, Asm& z, AsmNext& nx) {
        z.d_next = as_btw_dist(R + 1, nx.aA);
        as_btw_commit(nx.blA, z.d_next);
        nx.blA[0] = nx.blB[0]; nx.blA[1] = nx.blB[1]; nx.aA = nx.aB;
        as_btw_fetch(R + 3, nx.blB, nx.aB);
    };
    auto as_advance = [&](int R, Asm& z, AsmNext& nx) {
        z.D = z.Dn;
        z.O = z.On;
        z.d = z.d_next;
        if (((lo + R + 2) & (JT - 1)) == 0) {               // factor R+2 opens a new tile: the old one has been used up
            if constexpr (ASB) {
                // two-wave form: the NEXT tile waits in the registers of the eliminator wave (which has a hundred to spare; this
                // wave has none), and that wave puts it in place once it has seen row R committed -- i.e. the operands of
                // factor R+1, the last of the old tile, read.  The first four rows, committed before the eliminator starts,
                // fetch for themselves and wait for the memory.
                if (R < 4) {
                    as_tile_fetch(nx.k0_next, nx);
                    as_tile_commit(nx.k0_next, nx);
                    nx.k0_next += JT;
                } else {
                    nx.tiles_wanted++;
                    int spin = 0;
                    while (lds_peek(S + AS_FLAGS + 2) < (double)nx.tiles_wanted && ++spin < (1 << 22)) __builtin_amdgcn_s_sleep(1);
                    if (spin >= (1 << 22) && lane == 0) S[AS_FLAGS + 3] = 1.0;
                }
            } else {
            as_tile_commit(nx.k0_next, nx);
            nx.k0_next += JT;
            as_tile_fetch(nx.k0_next, nx);
            }
        }
    };

    // ---- H block row prefetch (HBM -> registers) and commit (registers -> LDS slot) ---------
    // (passed by value: captured-by-reference scalars ended up in scratch memory)
    struct HRow { double h0[2], h1[4], h2, h3, hx, hg; };
    const size_t hbase = base;      // the buffer of the window's current normal equations
    const double* __restrict__ Hbase = v.H + hbase * HROW;
    const double* __restrict__ gbase = v.gvec + hbase * 15;
    const double* __restrict__ zrow = v.zrow;
    double* __restrict__ Lbase = v.Lp + base * PANEL;
    constexpr size_t Lstride = PANEL;                 // doubles between consecutive keyframes of a window
    double* __restrict__ dbase = v.delta + base * 15;
    auto fetch_row = [=](int kk) {
        HRow r;
        const bool real = row_kind(kk) == 0;
        if (!rev) {
            // unconditional loads: a block that is absent (row outside the window, or reaching in front of it) is read
            // from a row of zeros -- wave-uniform pointer selects instead of per-lane predicates (exec juggling);
            // lanes beyond a block's extent read neighbouring words that commit_row sends to the write sink
            const double* Hk = real ? Hbase + (size_t)kk * HROW : zrow;
            const double* H1 = (real && kk >= 1) ? Hk + H_D1 : zrow;
            const double* H2 = (real && kk >= 2) ? Hk + H_D2 : zrow;
            const double* H3 = (real && kk >= 3) ? Hk + H_D3 : zrow;
            const double* HX = (real && kk == 2 && mp_third > 0.0) ? Hk + H_DX : zrow;   // only the marginal prior fills it
            const double* G0 = real ? gbase + (size_t)kk * 15 : zrow;
#pragma unroll
            for (int j = 0; j < 4; j++) r.h1[j] = H1[lane + 64 * j];
#pragma unroll
            for (int j = 0; j < 2; j++) r.h0[j] = Hk[H_D0 + lane + 64 * j];
            r.h2 = H2[lane];
            r.h3 = H3[lane];
            r.hx = HX[lane];
            r.hg = G0[lane];   // negated at commit (a use here would stall on vmcnt)
        } else {
            // reversed sequence: block d of row j couples j with j+d = H[j+d][d]^T (pose x pose for d >= 2).
            // Rows t, t+1, t+2 (kind 2) keep only their couplings to the reverse part (j+d >= t+3):
            // their diagonal blocks, mutual couplings and rhs belong to the forward sweep's window.
            const int kind = row_kind(kk);
            const bool has = kind == 0 || kind == 2;
            const int j = has ? n - 1 - (kk - qpad) : 0, back = kk - qpad;
            const double* Hj = Hbase + (size_t)j * HROW;
            const bool l1 = has && back >= 1 && j + 1 >= tsp + 3, l2 = has && back >= 2 && j + 2 >= tsp + 3,
                       l3 = has && back >= 3 && j + 3 >= tsp + 3;
#pragma unroll
            for (int jj = 0; jj < 2; jj++) r.h0[jj] = (real && lane + 64 * jj < 120) ? Hj[H_D0 + lane + 64 * jj] : 0.0;   // symmetric: as stored
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const bool in = lane + 64 * jj < 225;
                r.h1[jj] = (in && l1) ? Hj[HROW + H_D1 + cm_srcT[jj]] : 0.0;
            }
            r.h2 = (lane < 36 && l2) ? Hj[2 * HROW + H_D2 + s6_srcT] : 0.0;
            r.h3 = (lane < 36 && l3) ? Hj[3 * HROW + H_D3 + s6_srcT] : 0.0;
            r.hx = 0.0;
            r.hg = (real && lane < 15) ? gbase[(size_t)j * 15 + lane] : 0.0;
        }
        return r;
    };
    // Chunk sweeps: rows at a chunk boundary keep only the dof that belong to this chunk (vf_kernels.hpp "SEP").
    //   head (chunks c >= 1): sweep rows 0, 1 are keyframes whose pose dof sit in the LEFT separator: their pose rows
    //     and columns are pinned (identity), also in the blocks of rows 1..4 that reach back to them;
    //   tail (a separator follows): rows ni+1, ni+2 contribute their pose dof only (their velocity / bias dof are the
    //     head of the next chunk).
    // Applied when the row is committed -- never on the freshly prefetched values (that would stall on vmcnt).
    auto mask_boundary_row = [=](HRow r, int kk) {
        const bool head = CH && cg.i0 > 0 && kk <= 4, tail = CH && cg.has_sep && kk > cg.ni && kk <= cg.ni + 2;
#pragma unroll
        for (int j = 0; j < 2; j++) {            // diagonal block (lower triangle)
            const int a = t0_a[j], c = t0_c[j];
            const double ident = a == c ? 1.0 : 0.0;
            if (head && kk <= 1) r.h0[j] = (a >= 6 && c >= 6) ? r.h0[j] : ident;
            if (tail) r.h0[j] = (a < 6 && c < 6) ? r.h0[j] : ident;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {            // coupling to the keyframe in front
            const int idx = lane + 64 * j, a = idx / 15, c = idx - a * 15;
            if (head) {
                if (kk == 1) r.h1[j] = (a >= 6 && c >= 6) ? r.h1[j] : 0.0;
                if (kk == 2) r.h1[j] = c >= 6 ? r.h1[j] : 0.0;
            }
            if (tail) r.h1[j] = (kk == cg.ni + 1 ? a < 6 : (a < 6 && c < 6)) ? r.h1[j] : 0.0;
        }
        if (head) {
            if (kk == 2 || kk == 3) { r.h2 = 0.0; r.hx = 0.0; }   // pose x pose coupling to a pinned keyframe: carried by the spike
            if (kk == 3 || kk == 4) r.h3 = 0.0;
            if (kk <= 1 && lane < 6) r.hg = 0.0;
        }
        if (tail && lane >= 6) r.hg = 0.0;
        return r;
    };
    auto commit_row = [&](auto ph, const HRow r_in, int kind, int kk) {   // sweep row kk with kk & 3 == PH
        constexpr int PH = decltype(ph)::value;
        constexpr int s = PH * 15, c1 = ((PH + 3) & 3) * 15, c2 = ((PH + 2) & 3) * 15, c3 = ((PH + 1) & 3) * 15;
        HRow r = r_in;
        if constexpr (CH) {
            if ((cg.i0 > 0 && kk <= 4) || (cg.has_sep && kk > cg.ni && kk <= cg.ni + 2)) r = mask_boundary_row(r_in, kk);
        }
        if constexpr (CW) {
            // the words of a block row land in their blocks in the order they were loaded: no per-lane maps
            constexpr int base = PH * CW_SLOT;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const double d0 = r.h0[j] + (kind == 0 ? t0_lam[j] : (kind == 1 ? t0_one[j] : 0.0));
                S[lane + 64 * j < 120 ? base + CW_D0 + lane + 64 * j : S_DUMP + 32 + lane] = d0;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) S[lane + 64 * j < 225 ? base + CW_D1 + lane + 64 * j : S_DUMP + 32 + lane] = r.h1[j];
            S[lane < 36 ? base + CW_D2 + (lane / 6) * 15 + lane % 6 : S_DUMP + 32 + lane] = r.h2;
            S[lane < 54 ? base + CW_D2 + (lane / 9) * 15 + 6 + lane % 9 : S_DUMP + 32 + lane] = r.hx;
            S[lane < 36 ? base + CW_D3 + lane : S_DUMP + 32 + lane] = r.h3;
            S[lane < 15 ? S_GD + s + lane : S_DUMP + 32 + lane] = -r.hg;
            return;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const double d0 = r.h0[j] + (kind == 0 ? t0_lam[j] : (kind == 1 ? t0_one[j] : 0.0));
            S[t0_off[j] >= 0 ? S_WD + s * LDW + s + t0_off[j] : S_DUMP + 32 + lane] = d0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) S[cm_off[j] >= 0 ? S_WD + s * LDW + c1 + cm_off[j] : S_DUMP + 32 + lane] = r.h1[j];
        // pose rows against the keyframes two and three back: the 6x6 blocks, and columns 6..14 (zero, but for the
        // marginal prior's entries in the window's third row): the panel reads whole rows
        S[s6_off >= 0 ? S_WD + s * LDW + c2 + s6_off : S_DUMP + 32 + lane] = r.h2;
        S[x9_off >= 0 ? S_WD + s * LDW + c2 + x9_off : S_DUMP + 32 + lane] = r.hx;
        S[s6_off >= 0 ? S_WD + s * LDW + c3 + s6_off : S_DUMP + 32 + lane] = r.h3;
        S[x9_off >= 0 ? S_WD + s * LDW + c3 + x9_off : S_DUMP + 32 + lane] = 0.0;
        S[lane < 15 ? S_GD + s + lane : S_DUMP + 32 + lane] = -r.hg;
    };
    const int n4 = cnt;   // pivots of this sweep; identity rows beyond the real ones are eliminated harmlessly
    // byte offsets of this lane's panel entries within a keyframe's panel (forward sweep: lane 15 + r holds row r)
    unsigned pp_off[8];
#pragma unroll
    for (int c = 0; c < 7; c++) pp_off[c] = (unsigned)panel_pair_off(lane >= 15 && lane < 58 ? lane - 15 : 0, c);
    pp_off[7] = (unsigned)((PANEL_LAST + (lane >= 15 && lane < 58 ? lane - 15 : 0)) * sizeof(double));
#ifdef VF_SOLVE_STAMPS
    unsigned long long st[16] = {0}, tprev = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (MODE != SOLVE_CHUNK_BWD && !BWD && !INCB) {
    Asm az;
    AsmNext anx;
    if constexpr (AS) {
        az.D = az.O = az.Dfin = az.Z = az.On = az.Dn = (d4_t){0, 0, 0, 0};     // row 0 has no factor in front of it
        az.d = az.d_next = 0;
        anx.k0_next = (lo + 1) & ~(JT - 1);
        anx.tiles_wanted = 0;
        as_tile_fetch(anx.k0_next, anx);
        as_tile_commit(anx.k0_next, anx);
        anx.k0_next += JT;
        if constexpr (!ASB) as_tile_fetch(anx.k0_next, anx);
        { const double z2[2] = {0.0, 0.0}; as_btw_commit(z2, 0); }
        as_btw_fetch(1, anx.blA, anx.aA);
        as_btw_fetch(2, anx.blB, anx.aB);
        WSYNC();
        // one iteration outside the elimination loop: the first four rows (whatever the form), and every row of the assembler wave
        auto whole_row = [&](auto ph, auto special_, int R) {
            const int fimg = AS_LJ + ((lo + R + 1) & (JT - 1)) * LJS;
            as_piece(IC<0>{}, az, fimg);
            as_stage_btw(R, az, anx);
            as_piece(IC<2>{}, az, fimg);  as_piece(IC<3>{}, az, fimg);  as_piece(IC<4>{}, az, fimg);  as_piece(IC<5>{}, az, fimg);
            as_piece(IC<7>{}, az, fimg);  as_piece(IC<8>{}, az, fimg);  as_piece(IC<9>{}, az, fimg);
            as_piece(IC<10>{}, az, fimg); as_piece(IC<12>{}, az, fimg); as_piece(IC<13>{}, az, fimg);
            as_piece(IC<14>{}, az, fimg); as_piece(IC<15>{}, az, fimg); as_piece(IC<16>{}, az, fimg); as_piece(IC<17>{}, az, fimg);
            if constexpr (ASB && decltype(special_)::value == 0) {
                // the window may be touched once the eliminator has read pivot row R - 4 (its Schur write-back of the step
                // before is then done as well) and until it reads the accumulators of that step -- it waits for us there
                int spin = 0;
                while (lds_peek(S + AS_FLAGS) < (double)(R - 4) && ++spin < (1 << 22)) __builtin_amdgcn_s_sleep(1);
                if (spin >= (1 << 22) && lane == 0) S[AS_FLAGS + 3] = 1.0;      // (never seen: the eliminator reports it as a failed solve)
            }
            as_rmw(ph, az);
            as_commit(ph, special_, R, az);
            if constexpr (decltype(special_)::value == 0) as_late_prior(R);
            WSYNC();
            if constexpr (ASB) { if (lane == 0) S[AS_FLAGS + 1] = (double)R; }       // rows <= R are in the window
            as_advance(R, az, anx);
            WSYNC();
        };
        whole_row(IC<0>{}, IC<1>{}, 0);
        whole_row(IC<1>{}, IC<1>{}, 1);
        whole_row(IC<2>{}, IC<1>{}, 2);
        whole_row(IC<3>{}, IC<1>{}, 3);
        if constexpr (ASB) {
#pragma unroll 1
            for (int R = 4; R < cnt + 4; R += 4) {
                whole_row(IC<0>{}, IC<0>{}, R);
                whole_row(IC<1>{}, IC<0>{}, R + 1);
                whole_row(IC<2>{}, IC<0>{}, R + 2);
                whole_row(IC<3>{}, IC<0>{}, R + 3);
            }
            return;
        }
    } else if constexpr (ASA) {
        // the tile behind the one iteration 4 works on (factor lo + 5): ours to prefetch and to put in place from now on
        anx.k0_next = (((lo + 5) >> JT_LOG) + 1) << JT_LOG;
        anx.tiles_wanted = 0;
        as_tile_fetch(anx.k0_next, anx);
        int spin = 0;                  // the assembler wave commits the first four rows
        while (lds_peek(S + AS_FLAGS + 1) < 3.0 && ++spin < (1 << 22)) __builtin_amdgcn_s_sleep(1);
        if (spin >= (1 << 22)) failed = 1;
    } else {
    commit_row(IC<0>{}, fetch_row(0), row_kind(0), 0);
    commit_row(IC<1>{}, fetch_row(1), row_kind(1), 1);
    commit_row(IC<2>{}, fetch_row(2), row_kind(2), 2);
    commit_row(IC<3>{}, fetch_row(3), row_kind(3), 3);
    if constexpr (INCF) {
        // the sweep's trailing window as the elimination of the keyframes in front of keyframe cg.i0 left it: the 27 dof
        // [k: 15][k+1: pose][k+2: pose] and their rhs, over the rows just committed (slots 0 .. 2: sweep index 0 is phase 0)
        if (cg.i0 > 0) {
            const double* __restrict__ ckp = v.ck + (base >> CK_LOG) * CK_SZ;
            for (int e = lane; e < SEP * 28; e += 64) {
                const int i = e / 28, jc = e - i * 28;
                const int oi = i < 15 ? 0 : (i < 21 ? 1 : 2), ai = i < 15 ? i : (i < 21 ? i - 15 : i - 21);
                const int oj = jc < 15 ? 0 : (jc < 21 ? 1 : 2), aj = jc < 15 ? jc : (jc < 21 ? jc - 15 : jc - 21);
                const double val = ckp[e];
                if (jc == 27) S[S_GD + oi * 15 + ai] = val;
                else if (jc <= i) S[S_WD + (oi * 15 + ai) * LDW + oj * 15 + aj] = val;
            }
        }
    }
    }
    WSYNC();
    // ---- one elimination step, phase PH = k & 3 compile-time --------------------------------
    // `pend`, `pend2` = block rows of keyframes k+4, k+5 (fetched two steps and one step ago); this step fetches k+6.
    auto step = [&](auto ph, int k, HRow& pend, HRow& pend2) {
        constexpr int PH = decltype(ph)::value;
        STAMP(0);
        if constexpr (INCF) {
            // a checkpoint at every CK-th keyframe SLOT (sweeps of later updates start at other keyframes of the window, the
            // slot grid stays): keyframe k + j sits in slot (PH + j) & 3 of the window
            if (k > 0 && ((base + (size_t)k) & (CK - 1)) == 0) {
                double* __restrict__ ckp = v.ck + ((base + (size_t)k) >> CK_LOG) * CK_SZ;
                for (int e = lane; e < SEP * 28; e += 64) {
                    const int i = e / 28, jc = e - i * 28;
                    const int oi = i < 15 ? 0 : (i < 21 ? 1 : 2), ai = i < 15 ? i : (i < 21 ? i - 15 : i - 21);
                    double val;
                    if (jc == 27) val = S[S_GD + ((PH + oi) & 3) * 15 + ai];
                    else {
                        const int hi_i = i >= jc ? i : jc, lo_i = i >= jc ? jc : i;
                        const int oa = hi_i < 15 ? 0 : (hi_i < 21 ? 1 : 2), a = hi_i < 15 ? hi_i : (hi_i < 21 ? hi_i - 15 : hi_i - 21);
                        const int ob = lo_i < 15 ? 0 : (lo_i < 21 ? 1 : 2), bb = lo_i < 15 ? lo_i : (lo_i < 21 ? lo_i - 15 : lo_i - 21);
                        val = S[S_WD + (((PH + oa) & 3) * 15 + a) * LDW + ((PH + ob) & 3) * 15 + bb];
                    }
                    ckp[e] = val;
                }
            }
        }
        double p[15];
#pragma unroll
        for (int c = 0; c < 15; c++) p[c] = S[ri_ph[PH] + c];
        if constexpr (CW) {     // rows of keyframe k+3 (lanes 36..41) hold pose columns only: the 6 x 6 block has no columns 6..14
            const bool narrow = lane >= 36 && lane < 42;
#pragma unroll
            for (int c = 6; c < 15; c++) p[c] = narrow ? 0.0 : p[c];
        }
        if constexpr (ASA) {    // pivot row k is in registers (and the write-back of step k - 1 behind us): its slot and the rows of the window are the assembler's
            WSYNC();
            if (lane == 0) S[AS_FLAGS] = (double)k;
        }
        STAMP(1);
        // panel factorisation: straight-line code in a fixed issue order (tools/gen_pivot.py); a non-positive
        // pivot turns the last reciprocal into NaN / inf, tested once per step
        // (each scaled column's pivot-block entries go through LDS to come back replicated over the 16-lane rows; replicating
        // them by VALU lane swaps instead was bit-identical and slower, 2.76 -> 3.04 ms fused at 1 024 windows: NOTEBOOK.md 7)
        double pv_inv;
        const int pv_bcw = lane < 15 ? (RINGM ? S_BC_RING : S_BC) + lane : S_DUMP + 32 + lane;
        const int pv_bcr = (RINGM ? S_BC_RING : S_BC) + (lane & 15);
        // (assembling sweep: iteration k + 4 -- row k + 4 from the operands of factor k + 5 -- rides in the pivot code's places)
        const int as_fimg = AS_LJ + ((lo + k + 5) & (JT - 1)) * LJS;
        // (piece i -- the I of as_piece: 0 = operand reads, 2 .. 17 = one matrix instruction each, with gaps -- at place i, i.e. as
        // early as possible; every other place and as late as possible made no difference, nor did issuing all of them back
        // to back in front of the Schur update)
#undef VF_PIVOT_SLOT
#define VF_PIVOT_SLOT(i) do { if constexpr (AS) { as_piece(IC<(i)>{}, az, as_fimg); if constexpr ((i) == 1) as_stage_btw(k + 4, az, anx); if constexpr ((i) == 26) as_rmw(ph, az); VF_SB(); } } while (0)
#include "../vf_pivot_15.inc"
#undef VF_PIVOT_SLOT
#define VF_PIVOT_SLOT(i) do {} while (0)
        (void)as_fimg;
        if (!(pv_inv < 1e300)) failed = 1;
        // (two-wave form: ask now how far the assembler is -- the answer travels under the panel's LDS writes, and if row k + 4
        // is there already, which is the rule, the wait in front of the Schur update costs no LDS round trip.  lds_ask issues
        // the read and waits for nothing; the value is first used behind the lgkmcnt(0) that follows the panel's writes.)
        double as_seen = 0.0;
        if constexpr (ASA) as_seen = lds_ask(S + AS_FLAGS + 1);
        STAMP(2);
        // sub-panel + rhs -> LDS (MFMA operands); rows 15..57 -> HBM, one 128-B line per lane
        if constexpr (RINGM) {
            // slot PH still holds the panel of step k-4: wait until the follower has read it
            // (bounded, like every hand-shake of the two-wave sweep: a follower that never reports must end as a failed solve,
            // not as a wave that spins until the GPU is reset)
            if (follower) {
                int spin = 0;
                while (lds_peek(S + S_CONS) < (double)(k - 3) && lds_peek(S + S_RING_OUT) == 0.0 && ++spin < RING_SPIN_MAX) __builtin_amdgcn_s_sleep(1);
                if (spin >= RING_SPIN_MAX) { failed = 1; if (lane == 0) S[S_RING_OUT] = 1.0; }
            }
        }
#pragma unroll
        for (int c = 0; c < 15; c++) S[pw_off + PH * RSLOT + c] = p[c];
        if (lane >= 15 && lane < 58 && pivot_real(k)) {
            VF_GLOBAL char* Lk = uniform_gptr(Lbase + (size_t)kf_of(k) * Lstride);     // (the lane's place in each pair: pp_off)
#pragma unroll
            for (int c = 0; c < 7; c++) { d2_t t; t.x = p[2 * c]; t.y = p[2 * c + 1]; *(VF_GLOBAL d2_t*)(Lk + pp_off[c]) = t; }
            *(VF_GLOBAL double*)(Lk + pp_off[7]) = p[14];
        }
        WSYNC();
        if constexpr (RINGM) { if (lane == 0) S[S_PROG] = (double)(k + 1); }   // panel k is complete in its ring slot
        STAMP(3);
        if constexpr (ASA) {    // row k + 4 committed, the between terms it brings added to rows k + 1 .. k + 3
            int spin = 0;
            if (as_seen < (double)(k + 4))
                while (lds_peek(S + AS_FLAGS + 1) < (double)(k + 4) && ++spin < (1 << 22)) __builtin_amdgcn_s_sleep(1);
#ifdef VF_RING_WITHHOLD     // fault-injection build only (tools/variants/libvilfusion_withhold.so): window 1's eliminator is told, once,
            if (w == 1 && k == 8) spin = 1 << 22;          // that its assembler never answered
#endif
            if (spin >= (1 << 22)) failed = 1;
            if (((lo + k + 6) & (JT - 1)) == 0) {      // factor k + 6 opens a new tile, and the assembler has read the last operands of the old one
                as_tile_commit(anx.k0_next, anx);
                WSYNC();
                anx.tiles_wanted++;
                if (lane == 0) S[AS_FLAGS + 2] = (double)anx.tiles_wanted;
                anx.k0_next += JT;
                as_tile_fetch(anx.k0_next, anx);
            }
        }
        // Schur update on the matrix cores: acc[t] = P_Ti P_Tj^T for the 3 lower 16x16 tiles
        // (the trailing entries are the accumulator input and the A operands are negated: T - P P^T leaves the matrix
        // cores ready to be written back, no accumulator read-out + subtraction pass)
        double a0[4], a1[4], n0[4], n1[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { a0[q] = S[op0[q] + PH * RSLOT]; a1[q] = S[op1[q] + PH * RSLOT]; }
        d4_t acc0, acc1, acc2;
        int tg[12];
#pragma unroll
        for (int q = 0; q < 12; q++) {
            if constexpr (ASA) tg[q] = tgB[q] + (tgM[q] & 0xffff) * ((PH + (tgM[q] >> 16)) & 3);
            else tg[q] = tgt_ph[PH][q];
        }
#pragma unroll
        for (int r = 0; r < 4; r++) { acc0[r] = S[tg[r]]; acc1[r] = S[tg[4 + r]]; acc2[r] = S[tg[8 + r]]; }
#pragma unroll
        for (int q = 0; q < 4; q++) { n0[q] = -a0[q]; n1[q] = -a1[q]; }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(n0[q], a0[q], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(n1[q], a0[q], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(n1[q], a1[q], acc2, 0, 0, 0);
        }
        // While the twelve MFMAs run (64 cycles each on this part: the longest stretch of the step that needs no issue
        // slots), row k+4 is committed to the slot the pivot keyframe frees -- its panel is in registers, the operand and
        // accumulator reads above are ahead of these writes in the LDS queue, and the write-back below goes to other rows.
        if constexpr (AS) {
            as_commit(ph, IC<0>{}, k + 4, az);
            as_late_prior(k + 4);
            as_advance(k + 4, az, anx);          // (a dispatch on the phase around ONE copy of this was slower: the register copies where its four arms meet)
        } else if constexpr (ASA) {
            // (nothing to commit or to fetch: the partner wave does both)
        } else {
        commit_row(ph, pend, row_kind(k + 4), k + 4);
        pend = pend2;
        pend2 = fetch_row(k + 6);              // also in the shadow; two steps of slack for the HBM round trip
        }
        STAMP(4);
#pragma unroll
        for (int r = 0; r < 4; r++) { S[tg[r]] = acc0[r]; S[tg[4 + r]] = acc1[r]; S[tg[8 + r]] = acc2[r]; }
        WSYNC();
        STAMP(5);
    };
    {
        HRow pend = {}, pend2 = {};
        if constexpr (!AS && !ASA) { pend = fetch_row(4); pend2 = fetch_row(5); }
#pragma unroll 1
        for (int k = 0; k < n4; k += 4) {
            step(IC<0>{}, k, pend, pend2);
            step(IC<1>{}, k + 1, pend, pend2);
            step(IC<2>{}, k + 2, pend, pend2);
            step(IC<3>{}, k + 3, pend, pend2);
        }
    }
    }   // forward sweep
    if constexpr (MODE == SOLVE_FULL_FWD || AS || ASA || INCF) {
        if constexpr (ASA) { if (lds_peek(S + AS_FLAGS + 3) != 0.0) failed = 1; }     // a wait of the assembler wave ran out
        if (lane == 0) v.fail[w] = failed;
#ifdef VF_SOLVE_STAMPS
        if (w == 0 && lane == 0) { for (int i = 0; i < 6; i++) g_stamps[i] = st[i]; for (int i = 11; i < 16; i++) g_stamps[i] = st[i]; }
#endif
        return;
    }
    if constexpr (MODE == SOLVE_CHUNK_FWD) {
        // the cut keyframe and the two after it sit in slots 0..2 (cnt is a multiple of 4): the separator's 27 dof
        // (15 + pose + pose): own H + lambda + Schur terms of this chunk's interior, and rhs, go to sep_out [27][28]
        if (cg.has_sep) {
            for (int e = lane; e < SEP * 28; e += 64) {
                const int i = e / 28, jc = e - i * 28;
                const int oi = i < 15 ? 0 : (i < 21 ? 1 : 2), ai = i < 15 ? i : (i < 21 ? i - 15 : i - 21);
                double val;
                if (jc == 27) {
                    val = S[S_GD + oi * 15 + ai];
                } else {
                    const int hi_i = i >= jc ? i : jc, lo_i = i >= jc ? jc : i;
                    const int oa = hi_i < 15 ? 0 : (hi_i < 21 ? 1 : 2), a = hi_i < 15 ? hi_i : (hi_i < 21 ? hi_i - 15 : hi_i - 21);
                    const int ob = lo_i < 15 ? 0 : (lo_i < 21 ? 1 : 2), bb = lo_i < 15 ? lo_i : (lo_i < 21 ? lo_i - 15 : lo_i - 21);
                    val = S[S_WD + (oa * 15 + a) * LDW + ob * 15 + bb];
                }
                sep_out[e] = val;
            }
        }
        if (lane == 0 && failed) atomicOr(v.fail + w, 1);
        return;
    }

    // ---- back substitution: delta_k = L_kk^-T (y_k - sum_p L[p][k-cols]^T delta(p)) -----------
    // Panel rows in HBM: 0..26 sub-diagonal rows (p = 15..41), 27 = y, 28..42 = L_kk^-T.
    // Lane r < 43 holds row r in registers; rows 0..27 go through LDS for the column sums,
    // L^-T stays in the registers of lanes 28..42.  Panels are prefetched four steps ahead, each into the register
    // slot (k & 3) it is consumed from (three steps with a rotating triple measured 2.5 % slower under a full batch;
    // touching the lines further ahead with a dword load does not help: vector loads return in order).
    S[S_DL + lane] = 0.0;
    if constexpr (MODE == SOLVE_CHUNK_BWD) {
        WSYNC();
        // increments of the separator dof (solved by k_sep_solve) start the recursion; the velocity / bias dof of the
        // two keyframes after the cut belong to the next chunk and do not couple to this one
        if (cg.has_sep && lane < 45) S[S_DL + lane] = (lane < 15 || (lane % 15) < 6) ? dbase[(size_t)cg.ni * 15 + lane] : 0.0;
        WSYNC();
    }
    if constexpr (TW) {
        __syncthreads();   // both forward sweeps done; their trailing windows are in S (left) / S_other
        if (wave == 0) {
            // dense 45x45 system of keyframes t, t+1, t+2 = left window (original H of these rows +
            // left Schur terms) + right window (Schur terms only: its rows were committed as zeros,
            // reversed order => transposed blocks).  Only regions that are written are read.
            const int sR[3] = {((qpad + n - 1 - tsp) & 3) * 15, ((qpad + n - 2 - tsp) & 3) * 15, ((qpad + n - 3 - tsp) & 3) * 15};
            for (int e = lane; e < 45 * 46; e += 64) {
                const int i = e / 46, jc = e - i * 46;
                const int oi = i / 15, ai = i - oi * 15;
                double val;
                if (jc == 45) {
                    val = S[S_GD + oi * 15 + ai] + S_other[S_GD + sR[oi] + ai];
                } else {
                    const int hi_i = i >= jc ? i : jc, lo_i = i >= jc ? jc : i;     // symmetric: fill both triangles
                    const int oa = hi_i / 15, a = hi_i - oa * 15, ob = lo_i / 15, bb = lo_i - ob * 15;
                    double vl = 0.0, vr = 0.0;
                    if (oa - ob < 2 || a < 6) vl = S[S_WD + (oa * 15 + a) * LDW + ob * 15 + bb];
                    // right window: row = keyframe with the larger sweep index = the smaller keyframe (ob)
                    if (oa == ob) vr = S_other[S_WD + (sR[oa] + a) * LDW + sR[oa] + bb];
                    else if (oa - ob == 1 || bb < 6) vr = S_other[S_WD + (sR[ob] + bb) * LDW + sR[oa] + a];
                    val = vl + vr;
                }
                MID[i * MID_LD + jc] = val;
            }
            WSYNC();
            for (int c = 0; c < 45; c++) {       // Gaussian elimination (SPD: no pivoting), entry-parallel
                const double piv = MID[c * MID_LD + c];
                if (!(piv > 0.0)) failed = 1;
                const double inv = 1.0 / piv;
                const int m = 44 - c;
                for (int e = lane; e < m * (m + 1); e += 64) {
                    const int i = c + 1 + e / (m + 1), jc = c + 1 + (e - (e / (m + 1)) * (m + 1));
                    MID[i * MID_LD + jc] -= MID[i * MID_LD + c] * inv * MID[c * MID_LD + jc];
                }
                WSYNC();
            }
            for (int i = 44; i >= 0; i--) {      // back substitution on the upper triangle
                const double xi = MID[i * MID_LD + 45] / MID[i * MID_LD + i];
                if (lane < i) MID[lane * MID_LD + 45] -= MID[lane * MID_LD + i] * xi;
                if (lane == 0) MID[45 * MID_LD + i] = xi;
                WSYNC();
            }
            if (lane < 45) dbase[(size_t)tsp * 15 + lane] = MID[45 * MID_LD + lane];
        }
        __syncthreads();
        // increments of the keyframes just beyond this sweep's last pivot, in its own slot order
        if (!rev) {          // rows t (15), t+1, t+2 at sweep indices tsp, tsp+1, tsp+2 (tsp % 4 == 0)
            if (lane < 45) S[S_DL + lane] = MID[45 * MID_LD + lane];
        } else {             // sweep indices cnt, cnt+1, cnt+2 <-> keyframes t+2, t+1, t
            if (lane < 45) { const int o = lane / 15, a = lane - o * 15; S[S_DL + ((cnt + o) & 3) * 15 + a] = MID[45 * MID_LD + (2 - o) * 15 + a]; }
        }
        WSYNC();
    }
    struct PRow { d2_t x[8]; };
    constexpr int BWD_PD = 2;      // (2 against 4 slots: solve stage 3.44 against 3.48-3.50 ms at 1 024 windows, 178 against 240 registers; round 5)
    static_assert(BWD_PD == 2 || BWD_PD == 4, "the back substitution keeps 2 or 4 panel slots: any other depth reads panels it has not loaded");
    constexpr int PD = (MODE == SOLVE_FULL_BWD || INCB) ? BWD_PD : 4;      // panels prefetched ahead of the recursion (SOLVE_FULL_BWD1, one wave per SIMD: 4)
    // Backward sweep: lane r < 28 holds panel row r (sub-diagonal rows and the rhs row: they go through LDS); the rows of
    // L^-T sit in lanes XL .. XL+14 of ONE 16-lane row, where s and x are formed as well, so that both matrix-vector
    // products of the recursion broadcast their vector with DPP row_newbcast inside v_fmac_f64 (one instruction per term
    // instead of v_readlane x2, s_nop, v_fma); every other lane points at the keyframe's zero cell.
    constexpr int XL = 32;
    const bool xl_lane = lane >= XL && lane < XL + 15;
    unsigned pb_off[8];
    {
        const int brow = lane < 28 ? lane : (xl_lane ? 28 + (lane - XL) : -1);
#pragma unroll
        for (int c = 0; c < 7; c++) pb_off[c] = brow >= 0 ? (unsigned)panel_pair_off(brow, c) : (unsigned)(PANEL_DUMP * sizeof(double));
        pb_off[7] = (unsigned)((brow >= 0 ? PANEL_LAST + brow : PANEL_DUMP) * sizeof(double));
    }
    auto load_panel = [=](int k) {   // not a real pivot: any valid panel is loaded and zeroed at use (no use here: no stall)
        PRow r;
        const bool ok = k >= 0 && k < cnt && pivot_real(k);
        const VF_GLOBAL char* Lk = uniform_gptr(Lbase + (size_t)(ok ? kf_of(k) : 0) * Lstride);
#pragma unroll
        for (int c = 0; c < 7; c++) r.x[c] = *(const VF_GLOBAL d2_t*)(Lk + pb_off[c]);
        r.x[7].x = *(const VF_GLOBAL double*)(Lk + pb_off[7]);
        r.x[7].y = 0.0;
        return r;
    };
    const int bw_off = lane < 28 ? S_P + lane * 15 : S_DUMP + 16;
    const int col = xl_lane ? lane - XL : 0;
    const int dl_w = xl_lane ? S_DL + lane - XL : S_DUMP + 32 + lane;
    WSYNC();
    // Software-pipelined: the recursion delta_{k+1} -> delta_k runs on registers only --
    //   s = y - part - sum_a P[a][.] delta_{k+1}[a]   (delta_{k+1} = the previous step's x, broadcast by DPP)
    //   x = L_kk^-T s                                  (s broadcast by DPP)
    // while everything that does not depend on delta_{k+1} is prepared one step ahead (`prep`): the panel rows of the
    // next keyframe go through LDS into per-column registers, and the couplings to the two keyframes further on
    // (12 pose columns, increments already in LDS) are summed into `part`.  The step was 3 LDS round trips and an HBM
    // wait in sequence (about 2 600 cycles for 200 instructions); LDS accesses of one wave execute in issue order, so
    // the write -> read hand-offs below need a compiler barrier, not a wait.
#define CBAR() asm volatile("" ::: "memory")
    struct Col { double row[15], pv[15], y, part, dold; };   // of one keyframe, in lanes XL .. XL+14: its L^-T row, its column data
    int inc_run = 0;      // INCB: consecutive keyframes whose increment came out as it was
    auto prep = [&](auto ph, int k, PRow& slot, Col& o) {
        constexpr int PH = decltype(ph)::value;          // = k & 3
        constexpr int b2 = S_DL + ((PH + 2) & 3) * 15, b3 = S_DL + ((PH + 3) & 3) * 15;
        STAMP(6);
        const double keep = (k >= 0 && pivot_real(k)) ? 1.0 : 0.0;   // identity rows: zero panel
#pragma unroll
        for (int c = 0; c < 7; c++) { o.row[2 * c] = keep * slot.x[c].x; o.row[2 * c + 1] = keep * slot.x[c].y; }
        o.row[14] = keep * slot.x[7].x;
        if constexpr (INCB) o.dold = (xl_lane && k >= 0 && pivot_real(k)) ? dbase[(size_t)kf_of(k) * 15 + lane - XL] : 0.0;
        slot = load_panel(k - PD);   // PD steps ahead, into the slot just consumed (slot = k & (PD - 1): no register rotation)
#pragma unroll
        for (int c = 0; c < 15; c++) S[bw_off + c] = o.row[c];
        CBAR();
        STAMP(7);
#pragma unroll
        for (int a = 0; a < 15; a++) o.pv[a] = S[S_P + a * 15 + col];
        double q[12], d[12];
#pragma unroll
        for (int a = 0; a < 12; a++) q[a] = S[S_P + (15 + a) * 15 + col];
#pragma unroll
        for (int a = 0; a < 6; a++) { d[a] = S[b2 + a]; d[6 + a] = S[b3 + a]; }
        o.y = S[S_P + 27 * 15 + col];
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int a = 0; a < 12; a += 3) {
            t0 = fma(q[a], d[a], t0);
            t1 = fma(q[a + 1], d[a + 1], t1);
            t2 = fma(q[a + 2], d[a + 2], t2);
        }
        o.part = (t0 + t1) + t2;
        CBAR();                      // the next prep overwrites these panel rows in LDS
        STAMP(8);
    };
    auto solve = [&](auto ph, int k, const Col& c_, double& xprev) {
        constexpr int PH = decltype(ph)::value;
        STAMP(9);
        // acc += (lane XL + N of xsrc) * other, on the lanes of that 16-lane row (the DPP operand must have been written
        // at least two wait states earlier: s_nop in front of the first use of a fresh vector)
        auto bfma = [](auto n_, double& acc, const double bsrc, const double other) {
            constexpr int N = decltype(n_)::value;
            asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(bsrc), "v"(other), "n"(N));
        };
        double s0 = c_.part, s1 = 0.0, s2 = 0.0;
        asm volatile("s_nop 1" :: "v"(xprev));
        bfma(IC<0>{}, s0, xprev, c_.pv[0]);   bfma(IC<1>{}, s1, xprev, c_.pv[1]);   bfma(IC<2>{}, s2, xprev, c_.pv[2]);
        bfma(IC<3>{}, s0, xprev, c_.pv[3]);   bfma(IC<4>{}, s1, xprev, c_.pv[4]);   bfma(IC<5>{}, s2, xprev, c_.pv[5]);
        bfma(IC<6>{}, s0, xprev, c_.pv[6]);   bfma(IC<7>{}, s1, xprev, c_.pv[7]);   bfma(IC<8>{}, s2, xprev, c_.pv[8]);
        bfma(IC<9>{}, s0, xprev, c_.pv[9]);   bfma(IC<10>{}, s1, xprev, c_.pv[10]); bfma(IC<11>{}, s2, xprev, c_.pv[11]);
        bfma(IC<12>{}, s0, xprev, c_.pv[12]); bfma(IC<13>{}, s1, xprev, c_.pv[13]); bfma(IC<14>{}, s2, xprev, c_.pv[14]);
        const double s = c_.y - ((s0 + s1) + s2);
        // x = L^-T s on lanes XL .. XL+14 (row c of L^-T in registers)
        double x0 = 0.0, x1 = 0.0;
        asm volatile("s_nop 1" :: "v"(s));
        bfma(IC<0>{}, x0, s, c_.row[0]);   bfma(IC<1>{}, x1, s, c_.row[1]);   bfma(IC<2>{}, x0, s, c_.row[2]);   bfma(IC<3>{}, x1, s, c_.row[3]);
        bfma(IC<4>{}, x0, s, c_.row[4]);   bfma(IC<5>{}, x1, s, c_.row[5]);   bfma(IC<6>{}, x0, s, c_.row[6]);   bfma(IC<7>{}, x1, s, c_.row[7]);
        bfma(IC<8>{}, x0, s, c_.row[8]);   bfma(IC<9>{}, x1, s, c_.row[9]);   bfma(IC<10>{}, x0, s, c_.row[10]); bfma(IC<11>{}, x1, s, c_.row[11]);
        bfma(IC<12>{}, x0, s, c_.row[12]); bfma(IC<13>{}, x1, s, c_.row[13]); bfma(IC<14>{}, x0, s, c_.row[14]);
        const double x = x0 + x1;
        S[xl_lane ? S_DL + PH * 15 + lane - XL : dl_w] = x;
        // (head keyframes of a chunk: only their velocity / bias increments are this sweep's; the pose part is the separator's)
        if (xl_lane && pivot_real(k) && !(CH && cg.i0 > 0 && k < 2 && lane < XL + 6)) dbase[(size_t)kf_of(k) * 15 + lane - XL] = x;
        if constexpr (INCB) {
            const bool moved = xl_lane && pivot_real(k) && fabs(x - c_.dold) > v.wildfire;
            inc_run = __builtin_amdgcn_ballot_w64(moved) != 0 ? 0 : inc_run + 1;
        }
        xprev = x;
        STAMP(10);
    };
    {
        // (split back substitution: two waves per SIMD hide the HBM round trip between them; two panels in flight instead
        // of four keep the kernel inside the 256 registers that takes)
        PRow p3 = load_panel(n4 - 1), p2 = load_panel(n4 - 2), p1s, p0s;
        if constexpr (PD == 4) { p1s = load_panel(n4 - 3); p0s = load_panel(n4 - 4); }
        PRow& p1 = PD == 4 ? p1s : p3;
        PRow& p0 = PD == 4 ? p0s : p2;
        // increment of the keyframe after the last pivot (slot n4 & 3 = 0): zero, or the separator's / the middle system's
        double xprev = S[xl_lane ? S_DL + lane - XL : S_ZERO];
        Col ca, cb;
        if constexpr (MODE == SOLVE_FULL_BWD || INCB) {
            // two waves per SIMD: the partner wave covers this one's LDS round trips, so the recursion is not software-
            // pipelined here -- one set of column registers instead of two keeps the kernel inside 256 registers.  (A batch of
            // at most one window per SIMD has no partner wave: it takes SOLVE_FULL_BWD1, the pipelined loop below.)
            int stop_at = 0;
#pragma unroll 1
            for (int k = n4 - 1; k >= 3; k -= 4) {
                prep(IC<3>{}, k, p3, ca);
                solve(IC<3>{}, k, ca, xprev);
                prep(IC<2>{}, k - 1, p2, ca);
                solve(IC<2>{}, k - 1, ca, xprev);
                prep(IC<1>{}, k - 2, p1, ca);
                solve(IC<1>{}, k - 2, ca, xprev);
                prep(IC<0>{}, k - 3, p0, ca);
                solve(IC<0>{}, k - 3, ca, xprev);
                if constexpr (INCB) {
                    // keyframes k-3 .. k-1 came out as they were and every panel in front of k-3 is the old one (cg.ni: the first
                    // keyframe the forward sweep eliminated again): so would every increment in front of them
                    if (inc_run >= 3 && k - 3 <= cg.ni) { stop_at = k - 3; break; }
                }
            }
            if constexpr (INCB) { if (lane == 0) v.inc_stop[w] = lo + stop_at; }
        } else {
        prep(IC<3>{}, n4 - 1, p3, ca);
#pragma unroll 1
        for (int k = n4 - 1; k >= 3; k -= 4) {
            prep(IC<2>{}, k - 1, p2, cb);
            solve(IC<3>{}, k, ca, xprev);
            prep(IC<1>{}, k - 2, p1, ca);
            solve(IC<2>{}, k - 1, cb, xprev);
            prep(IC<0>{}, k - 3, p0, cb);
            solve(IC<1>{}, k - 2, ca, xprev);
            prep(IC<3>{}, k - 4, p3, ca);
            solve(IC<0>{}, k - 3, cb, xprev);
        }
        }
    }
#undef CBAR
#ifdef VF_SOLVE_STAMPS
    if (w == 0 && lane == 0) for (int i = (BWD ? 6 : 0); i < (BWD ? 11 : 16); i++) g_stamps[i] = st[i];
#endif
    if constexpr (MODE == SOLVE_FULL) { if (lane == 0) v.fail[w] = failed; }
    else if constexpr (!BWD && !INCB) { if (lane == 0 && failed) atomicOr(v.fail + w, 1); }
}
