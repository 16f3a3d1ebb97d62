// kernels/k4_band.inc -- K4: the kernels around band_solve_body (k4_band_body.inc): whole-window sweeps, the split and assembling forms,
// the two-wave assembling sweep and its role assignment, the incremental suffix sweep.
// A section of vf_kernels.hip (ONE translation unit); included from there, inside namespace vf, never compiled by itself.
__global__ void __launch_bounds__(64) k_band_solve(View v) {
    const int w = sweep_window(v, blockIdx.x);
    if (w < 0 || v.hi[w] - v.lo[w] <= 0 || window_done(v, w) || gated_off(v)) return;
    __shared__ double S[S_TOTAL];
    band_solve_body<SOLVE_FULL>(v, S, nullptr, nullptr, w, threadIdx.x, 0);
}

// the split form (see SOLVE_FULL_FWD / SOLVE_FULL_BWD)
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ void __launch_bounds__(64) k_band_forward(View v) {
    const int w = sweep_window(v, blockIdx.x);
    if (w < 0 || v.hi[w] - v.lo[w] <= 0 || window_done(v, w) || gated_off(v)) return;
    __shared__ double S[CW_TOTAL];
    band_solve_body<SOLVE_FULL_FWD>(v, S, nullptr, nullptr, w, threadIdx.x, 0);
}
// the assembling form (see SOLVE_ASM_FWD): one wave per SIMD, 39.7 KB of LDS; followed by k_band_backward
__attribute__((amdgpu_waves_per_eu(1, 1)))
__global__ void __launch_bounds__(64) k_band_forward_asm(View v) {
    const int w = sweep_window(v, blockIdx.x);
    if (w < 0 || v.hi[w] - v.lo[w] <= 0 || window_done(v, w) || gated_off(v)) return;
    __shared__ __attribute__((aligned(16))) double S[AS_TOTAL];
    band_solve_body<SOLVE_ASM_FWD>(v, S, nullptr, nullptr, w, threadIdx.x, 0);
}
// the same as two waves per window: eliminator + assembler on one LDS image (SOLVE_ASM_A / SOLVE_ASM_B).  (Each role alone
// fits the 256 registers a wave may have at two waves per SIMD -- 225 + 24 and 205 + 40; inlined into one kernel the allocator
// takes all 256 as VGPRs and spills 17 to scratch unless it is told to keep some of the budget as AGPRs.)
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ void __launch_bounds__(128) k_band_forward_asm2(View v, int w0) {
    const int w = sweep_window(v, w0 + blockIdx.x);
    if (w < 0 || v.hi[w] - v.lo[w] <= 0 || window_done(v, w) || gated_off(v)) return;
    __shared__ __attribute__((aligned(16))) double S[AS2_TOTAL];
    // Roles.  Every SIMD should hold ONE eliminator and one assembler: the two roles of two windows share its float64 units,
    // and two eliminators on one SIMD are two critical paths in each other's way (the same kernel on the same windows: 2.56 ms
    // balanced, 3.10-3.20 ms not).  Which SIMDs the two waves of a workgroup land on follows the dispatcher's round-robin state,
    // i.e. whatever the PREVIOUS kernel left behind: after k_decide the four workgroups of a CU come out as (0, 2), (1, 3), (2, 1),
    // (3, 0) and "wave 0 eliminates" is balanced; after the gated-off K3 launch of the hybrid solve, or in another process, it
    // is not (tools/archive/trace_context.py; a placement kernel in front moved the step between 23.3 and 26.7 ms).
    // So the workgroups of a CU agree among themselves: each claims, in a per-CU bit mask (View::place, cleared by the launch),
    // the SIMD of its wave 0 for its eliminator, or -- that one taken -- the SIMD of its wave 1, and swaps its roles then.  The
    // waves of a CU's workgroups form cycles over its four SIMDs (two waves each), so the greedy claim ends with one eliminator
    // per SIMD whatever the order of arrival.
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < 4) S[AS_FLAGS + threadIdx.x] = threadIdx.x < 2 ? -1.0 : 0.0;
    int swapped = 0;
    {
        const unsigned hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));      // HW_ID: simd [5:4], cu [11:8], sh [12], se [15:13]
        const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));     // XCC_ID [3:0]
        if (lane == 0) S[AS_FLAGS + 4 + wave] = (double)((hw >> 4) & 3);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int s0 = (int)S[AS_FLAGS + 4], s1 = (int)S[AS_FLAGS + 5];
            unsigned* cell = v.place + ((xcc & 7) << 8 | ((hw >> 8) & 0xff));               // (xcc, se, sh, cu)
            int sw = 0;
            if (s0 != s1) {
                const unsigned o0 = atomicOr(cell, 1u << s0);
                if (o0 & (1u << s0)) {
                    const unsigned o1 = atomicOr(cell, 1u << s1);
                    sw = (o1 & (1u << s1)) ? 0 : 1;
                }
            }
            S[AS_FLAGS + 6] = (double)sw;
        }
        __syncthreads();
        swapped = __builtin_amdgcn_readfirstlane((int)S[AS_FLAGS + 6]);
        if (VF_ASM2_ROLES == 2) swapped = 1;          // (test build: wave 1 eliminates in every workgroup)
    }
    const bool eliminator = (wave == 0) != (swapped != 0);
    // Issue priority to the eliminator: its steps are the critical path, the assembler has 40 % slack, and the two share one
    // SIMD's float64 units (DESIGN.md 7.16: solve 3.66 -> 3.50 ms at 1 024 windows; priority to the assembler instead was
    // 3.63, to neither 3.66)
    if (eliminator) __builtin_amdgcn_s_setprio(3);
    if (eliminator) band_solve_body<SOLVE_ASM_A>(v, S, nullptr, nullptr, w, lane, 0);
    else band_solve_body<SOLVE_ASM_B>(v, S, nullptr, nullptr, w, lane, 0);
}
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ void __launch_bounds__(64) k_band_backward(View v) {
    const int w = sweep_window(v, blockIdx.x);
    if (w < 0 || v.hi[w] - v.lo[w] <= 0 || window_done(v, w) || gated_off(v)) return;
    // the back substitution touches nothing of the trailing window [0, S_GD + 64): its LDS starts at the write sink
    __shared__ double Sb[S_TOTAL - S_DUMP];
    band_solve_body<SOLVE_FULL_BWD>(v, Sb - S_DUMP, nullptr, nullptr, w, threadIdx.x, 0);
}
// the same for batches of at most one window per SIMD (SolvePlan::bwd_one_wave), where a wave has no partner to cover its LDS round
// trips: the software-pipelined recursion of the fused kernel (two sets of column registers, four panels in flight), which
// needs more than the 256 registers of two waves per SIMD and gets them at one
__attribute__((amdgpu_waves_per_eu(1, 1)))
__global__ void __launch_bounds__(64) k_band_backward_1w(View v) {
    const int w = sweep_window(v, blockIdx.x);
    if (w < 0 || v.hi[w] - v.lo[w] <= 0 || window_done(v, w) || gated_off(v)) return;
    __shared__ double Sb[S_TOTAL - S_DUMP];
    band_solve_body<SOLVE_FULL_BWD1>(v, Sb - S_DUMP, nullptr, nullptr, w, threadIdx.x, 0);
}

// incremental updates (View::inc_*): the suffix of the window from the checkpoint in front of the first changed keyframe
__global__ void __launch_bounds__(64) k_inc_forward(View v) {
    const int w = blockIdx.x;
    const int lo = v.lo[w], hi = v.hi[w];
    if (hi - lo <= 0) return;
    const int m = inc_start(v.inc_k[w], lo);
    if (threadIdx.x == 0) v.inc_from[w] = m < hi ? m : hi;
    if (m >= hi) { if (threadIdx.x == 0) v.fail[w] = 0; return; }      // nothing changed: the factorisation stands
    __shared__ double S[S_TOTAL];
    band_solve_body<SOLVE_INC_FWD>(v, S, nullptr, nullptr, w, threadIdx.x, 0, ChunkGeom{m - lo, 0, 0});
}
__global__ void __launch_bounds__(64) k_inc_backward(View v) {
    const int w = blockIdx.x;
    const int lo = v.lo[w], hi = v.hi[w];
    if (hi - lo <= 0) return;
    const int m = inc_start(v.inc_k[w], lo);
    if (m >= hi) { if (threadIdx.x == 0) v.inc_stop[w] = hi; return; }
    __shared__ double Sb[S_TOTAL - S_DUMP];
    band_solve_body<SOLVE_INC_BWD>(v, Sb - S_DUMP, nullptr, nullptr, w, threadIdx.x, 0, ChunkGeom{0, m - lo, 0});
}

// two waves per window (see band_solve_body); windows shorter than 32 keyframes are left to wave 0 alone
__global__ void __launch_bounds__(128) k_band_solve_tw(View v) {
    const int w = blockIdx.x;
    const int n = v.hi[w] - v.lo[w];
    if (n <= 0 || window_done(v, w)) return;
    __shared__ double S2[2 * S_TOTAL];
    __shared__ double MID[MID_TOTAL];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (n < 32) {
        if (wave == 0) band_solve_body<SOLVE_FULL>(v, S2, nullptr, nullptr, w, lane, 0);
        return;
    }
    band_solve_body<SOLVE_TWISTED>(v, S2 + wave * S_TOTAL, S2 + (1 - wave) * S_TOTAL, MID, w, lane, wave);
}
