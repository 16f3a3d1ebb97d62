// kernels/launch.inc -- launchers (vf_kernels.hpp).
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ launchers
static inline unsigned nblk(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

void launch_preintegrate(const View& v, long g0, int n, const int* off, const double* steps, const double* bhat6,
                         const ImuCov& prm, int* status, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_preintegrate_t<false>, dim3(n), dim3(256), 0, s, v, g0, n, off, steps, bhat6,
                                  (const int*)nullptr, (const double*)nullptr, prm, status);
}
void launch_ingest_tail(const View& v, const int* off, const double* steps, const int* tail_a, const double* tail_btw,
                        const ImuCov& prm, int* status, hipStream_t s) {
    hipLaunchKernelGGL(k_preintegrate_t<true>, dim3(v.B), dim3(256), 0, s, v, 0L, v.B, off, steps, (const double*)nullptr, tail_a,
                       tail_btw, prm, status);
}
void launch_linearize_extra(const View& v, int which, hipStream_t s) {
    if (v.x_max <= 0) return;
    // (an engine that holds far losses, View::x_loss, launches the instance that reads them: chosen here, as K2's is below)
    if (v.x_loss) hipLaunchKernelGGL(k_linearize_extra<true>, dim3(nblk((long)v.B * v.x_max, 64)), dim3(64), 0, s, v, which);
    else hipLaunchKernelGGL(k_linearize_extra<false>, dim3(nblk((long)v.B * v.x_max, 64)), dim3(64), 0, s, v, which);
}
void launch_extra_gradient(const View& v, hipStream_t s) {
    if (v.x_max > 0) hipLaunchKernelGGL(k_extra_gradient, dim3(v.B), dim3(64), 0, s, v);
}
void launch_extra_rhs(const View& v, int slot, int row, double* gtmp, hipStream_t s) {
    hipLaunchKernelGGL(k_extra_rhs, dim3(nblk(v.B, 64)), dim3(64), 0, s, v, slot, row, gtmp);
}
void launch_extra_combine(const View& v, const double* Zm, size_t zstride, int slots, hipStream_t s) {
    if (far_big_form(v, slots)) {
        hipLaunchKernelGGL(k_extra_fill, dim3((unsigned)slots, (unsigned)v.B), dim3(256), 0, s, v, Zm, zstride, slots);
        hipLaunchKernelGGL(k_extra_combine<true>, dim3(v.B), dim3(1024), 0, s, v, Zm, zstride, slots);
        hipLaunchKernelGGL(k_extra_apply<true>, dim3(nblk((long)v.M * 15, 256), (unsigned)v.B), dim3(256), 0, s, v, Zm, zstride, slots);
    } else {
        hipLaunchKernelGGL(k_extra_combine<false>, dim3(v.B), dim3(256), 0, s, v, Zm, zstride, slots);
        hipLaunchKernelGGL(k_extra_apply<false>, dim3(nblk((long)v.M * 15, 256), (unsigned)v.B), dim3(256), 0, s, v, Zm, zstride, slots);
    }
}
static void launch_linearize_all(const View& v, const int* btw_kind, int which, hipStream_t s) {
    const int nb_imu = (int)nblk(v.G, K1_BLOCK), nb_btw = nb_imu, nb_pri = (int)nblk(v.B, K1_BLOCK);
    // (an engine that holds absolute factors launches the instances that read the slots' kinds, one that holds losses the ones
    // that read those, any other what it always has: chosen here, on the host)
    if (btw_kind) hipLaunchKernelGGL(k_linearize_all_abs, dim3(nb_imu + nb_btw + nb_pri), dim3(K1_BLOCK), 0, s, v, which, nb_imu, nb_btw, btw_kind);
    else if (v.btw_loss) hipLaunchKernelGGL(k_linearize_all_robust, dim3(nb_imu + nb_btw + nb_pri), dim3(K1_BLOCK), 0, s, v, which, nb_imu, nb_btw);
    else if (v.sh_G > 1) hipLaunchKernelGGL(k_linearize_all<true>, dim3(nb_imu + nb_btw + nb_pri), dim3(K1_BLOCK), 0, s, v, which, nb_imu, nb_btw);
    else hipLaunchKernelGGL(k_linearize_all<false>, dim3(nb_imu + nb_btw + nb_pri), dim3(K1_BLOCK), 0, s, v, which, nb_imu, nb_btw);
}
void launch_linearize_imu(const View& v, int which, hipStream_t s) {
    hipLaunchKernelGGL(k_linearize_imu, dim3(nblk(v.G, K1_BLOCK)), dim3(K1_BLOCK), 0, s, v, which);
}
void launch_linearize_between(const View& v, const int* btw_kind, int which, hipStream_t s) {
    if (btw_kind) hipLaunchKernelGGL(k_linearize_between_abs, dim3(nblk(v.G, 256)), dim3(256), 0, s, v, which, btw_kind);
    else if (v.btw_loss) hipLaunchKernelGGL(k_linearize_between_robust, dim3(nblk(v.G, 256)), dim3(256), 0, s, v, which);
    else hipLaunchKernelGGL(k_linearize_between, dim3(nblk(v.G, 256)), dim3(256), 0, s, v, which);
}
static void launch_linearize_between_prior(const View& v, const int* btw_kind, int which, hipStream_t s) {     // K2 + K2b in one launch
    const int nb_pri = (int)nblk(v.B, 64);
    if (btw_kind) hipLaunchKernelGGL(k_linearize_between_prior_abs, dim3(nblk(v.G, 256) + nb_pri), dim3(256), 0, s, v, which, nb_pri, btw_kind);
    else if (v.btw_loss) hipLaunchKernelGGL(k_linearize_between_prior_robust, dim3(nblk(v.G, 256) + nb_pri), dim3(256), 0, s, v, which, nb_pri);
    else hipLaunchKernelGGL(k_linearize_between_prior, dim3(nblk(v.G, 256) + nb_pri), dim3(256), 0, s, v, which, nb_pri);
}
void launch_linearize(const View& v, const int* btw_kind, int which, hipStream_t s) {
    if (v.B <= 128 || v.sh_G > 1) launch_linearize_all(v, btw_kind, which, s);
    else {
        launch_linearize_imu(v, which, s);
        launch_linearize_between_prior(v, btw_kind, which, s);
    }
}
void launch_linearize_tail(const View& v, const int* btw_kind, int nslid, hipStream_t s) {
    if (btw_kind) hipLaunchKernelGGL(k_linearize_tail_abs, dim3(2 * v.B + nblk(v.B, 64)), dim3(K1_BLOCK), 0, s, v, nslid, btw_kind);
    else if (v.btw_loss) hipLaunchKernelGGL(k_linearize_tail_robust, dim3(2 * v.B + nblk(v.B, 64)), dim3(K1_BLOCK), 0, s, v, nslid);
    else hipLaunchKernelGGL(k_linearize_tail, dim3(2 * v.B + nblk(v.B, 64)), dim3(K1_BLOCK), 0, s, v, nslid);
}
// K3 for the partitioned half of a hybrid solve whose sweep half assembles its own rows (see k_assemble)
void launch_assemble_for_partitioned(const View& v, hipStream_t s) {
    const View a = hybrid_half(v, 2);
    hipLaunchKernelGGL(k_assemble, dim3((unsigned)(v.M / AT), (unsigned)v.B), dim3(K3_NT), 0, s, a);
}
void launch_assemble(const View& v, hipStream_t s) {
    // (persistent forms were measured slower: one workgroup per CU with the next tile's loads in flight 5.1 ms, a plain
    // tile loop on 1024-2048 workgroups 4.0-4.3 ms, against 2.7 ms for one workgroup per tile -- stores count in vmcnt
    // on this ISA, so a loop waits for its own H stores before it can use the next tile's loads)
    hipLaunchKernelGGL(k_assemble, dim3((unsigned)(v.M / AT), (unsigned)v.B), dim3(K3_NT), 0, s, v);
}
void launch_assemble_window(const View& v, int window, hipStream_t s) {
    const View a = one_window_k3(v, window);
    hipLaunchKernelGGL(k_assemble, dim3((unsigned)(v.M / AT), 1u), dim3(K3_NT), 0, s, a);
}
void launch_partitioned_local(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_chunk_forward, dim3((unsigned)v.B * (unsigned)v.P), dim3(128), 0, s, v);
}
void launch_partitioned_global(const View& v, hipStream_t s) {
    const unsigned nb = (unsigned)v.B * (unsigned)v.P;
    hipLaunchKernelGGL(k_sep_solve, dim3(v.B), dim3(256), 0, s, v);
    hipLaunchKernelGGL(k_chunk_rhs, dim3(nb), dim3(256), 0, s, v);
    hipLaunchKernelGGL(k_chunk_back, dim3(nb), dim3(64), 0, s, v);
}
void launch_partitioned_solve(const View& v, hipStream_t s) {
    launch_partitioned_local(v, s);
    launch_partitioned_global(v, s);
}
// time-sharded windows, after the back substitution: zero the increments of the keyframes this rank does not own and put
// this rank's solve-failure flags behind them, so that ONE all-reduce (sum) leaves every rank with all increments and
// with the number of ranks whose elimination failed
__global__ void __launch_bounds__(256) k_mask_delta(View v) {
    const long gk = (long)blockIdx.x * 256 + threadIdx.x;
    if (gk < v.B) v.delta[(size_t)v.G * 15 + gk] = v.fail[gk] ? 1.0 : 0.0;
    if (gk >= v.G) return;
    const int w = (int)(gk / v.M), k = (int)(gk - (long)w * v.M);
    const int lo = v.lo[w];
    if (k < lo || k >= v.hi[w]) return;
    int klo, khi;
    own_range(v, w, klo, khi);
    if (k - lo >= klo && k - lo < khi) return;
#pragma unroll
    for (int a = 0; a < 15; a++) v.delta[(size_t)gk * 15 + a] = 0.0;
}
void launch_mask_delta(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_mask_delta, dim3(nblk(v.G, 256)), dim3(256), 0, s, v);
}
static void launch_asm2(const View& v, hipStream_t s) {
    // one launch per 1 024 windows -- the workgroups the part holds at once (4 per CU).  As ONE grid of 2 048 workgroups
    // the second thousand, dispatched one by one into the slots the first leaves, ran 1.7x slower than the first
    // (9.0 ms against 7.1 for the two launches; no such effect on the one-wave kernels)
    for (int w0 = 0; w0 < v.B; w0 += ASM2_CHUNK) {
        const unsigned nb = (unsigned)(v.B - w0 < ASM2_CHUNK ? v.B - w0 : ASM2_CHUNK);
        (void)hipMemsetAsync(v.place, 0, PLACE_CELLS * sizeof(unsigned), s);      // the per-CU claims of this launch
        hipLaunchKernelGGL(k_band_forward_asm2, dim3(nb), dim3(128), 0, s, v, w0);
    }
}
// the forward half of a split or assembling sweep (launch_band_factor: all there is of it)
static void launch_band_forward(const View& v, Sweep f, hipStream_t s) {
    if (f == Sweep::asm2) launch_asm2(v, s);
    else if (f == Sweep::asm1) hipLaunchKernelGGL(k_band_forward_asm, dim3(v.B), dim3(64), 0, s, v);
    else hipLaunchKernelGGL(k_band_forward, dim3(v.B), dim3(64), 0, s, v);
}
void launch_band_solve(const View& v, const View& vp, const SolvePlan& plan, hipStream_t s) {
    const View a = plan.hybrid() ? hybrid_half(v, 1) : v, b = plan.hybrid() ? hybrid_half(vp, 2) : vp;
    // few windows: two waves per window from both ends (latency); many: one wave per window (throughput).  (a.act, when the
    // engine hands it to a hybrid's sweep: the active windows are visited first)
    switch (plan.sweep) {
        case Sweep::none: break;
        case Sweep::two_sided: hipLaunchKernelGGL(k_band_solve_tw, dim3(a.B), dim3(128), 0, s, a); break;
        case Sweep::fused: hipLaunchKernelGGL(k_band_solve, dim3(a.B), dim3(64), 0, s, a); break;
        case Sweep::split:
        case Sweep::asm1:
        case Sweep::asm2:
            launch_band_forward(a, plan.sweep, s);
            if (plan.bwd_one_wave) hipLaunchKernelGGL(k_band_backward_1w, dim3(a.B), dim3(64), 0, s, a);
            else hipLaunchKernelGGL(k_band_backward, dim3(a.B), dim3(64), 0, s, a);
            break;
    }
    if (plan.partitioned) launch_partitioned_solve(b, s);
}
// windows of the running solve that still take LM trials (termination rule on)
__global__ void __launch_bounds__(1024) k_count_active(View v) {
    // ... and their compacted list, in window order (a block-wide inclusive scan per 1024 windows)
    __shared__ int scan[1024];
    __shared__ int base;
    const int tid = threadIdx.x;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int w0 = 0; w0 < v.B; w0 += 1024) {
        const int w = w0 + tid;
        const int on = (w < v.B && v.hi[w] > v.lo[w] && !v.done[w]) ? 1 : 0;
        scan[tid] = on;
        __syncthreads();
        for (int st = 1; st < 1024; st <<= 1) {
            const int add = tid >= st ? scan[tid - st] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        if (on && v.act) v.act[base + scan[tid] - 1] = w;
        __syncthreads();
        if (tid == 0) base += scan[1023];
        __syncthreads();
    }
    if (tid == 0) *v.n_active = base;
}
void launch_count_active(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_count_active, dim3(1), dim3(1024), 0, s, v);
}
void launch_model_change(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_model_change, dim3(v.B), dim3(256), 0, s, v);
}
void launch_retract(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_retract, dim3(nblk(v.G, 256)), dim3(256), 0, s, v);
}
void launch_reset_lambda(const View& v, const double* lambda0, int clear_done, hipStream_t s) {
    hipLaunchKernelGGL(k_reset_lambda, dim3(nblk(v.B, 256)), dim3(256), 0, s, v, lambda0, clear_done);
}
void launch_close_excursions(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_close_excursion, dim3(v.B), dim3(v.B <= 64 ? 1024 : 256), 0, s, v);
}
void launch_decide(const View& v, int init, hipStream_t s) {
    hipLaunchKernelGGL(k_decide, dim3(v.B), dim3(v.B <= 64 ? 1024 : 256), 0, s, v, init);
}
void launch_predict(const View& v, int window, int k0, int n, int from_trial, hipStream_t s) {
    if (window >= 0) hipLaunchKernelGGL(k_predict, dim3(1), dim3(1), 0, s, v, window, k0, n, from_trial);
    else hipLaunchKernelGGL(k_predict, dim3(nblk(v.B, 64)), dim3(64), 0, s, v, window, k0, n, from_trial);
}
void launch_relinearize(const View& v, double threshold, hipStream_t s) {
    hipLaunchKernelGGL(k_relinearize, dim3(nblk(v.G, 256)), dim3(256), 0, s, v, threshold);
}
__global__ void k_set_range(View v, int window, int lo, int hi) {
    if (lo >= 0) v.lo[window] = lo;
    v.hi[window] = hi;
}
__global__ void k_bump_lo(View v) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < v.B) v.lo[w] += 1;
}
__global__ void __launch_bounds__(64) k_put_between(View v, long g, int a, BtwArg rec) {
    const int f = threadIdx.x;
    if (f < BTW_IN) v.btw_in[(size_t)(g >> 6) * BTW_IN * TILE + (size_t)f * TILE + (g & 63)] = rec.r[f];
    if (f == 0) v.btw_a[g] = a;
}
// the loss of up to four band between factors of one window (vf_engine_set_between_loss on an asynchronous engine; NONE: what the
// staging calls put behind a record they write)
__global__ void __launch_bounds__(64) k_put_between_loss(View v, BtwLossArg a) {
    const int i = threadIdx.x;
    if (i < a.n) { v.btw_loss[a.g[i]] = a.loss[i]; v.btw_loss_k[a.g[i]] = a.k[i]; }
}
// ... and NONE for the slot behind every window's end: the record vf_engine_ingest_tail has just written there is a new factor
// (... and its kind on an engine that holds kinds: btw_kind, null elsewhere)
__global__ void __launch_bounds__(64) k_reset_tail_loss(View v, int* btw_kind) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= v.B || v.hi[w] >= v.M) return;
    const long g = (long)w * v.M + v.hi[w];
    v.btw_loss[g] = LOSS_NONE;
    v.btw_loss_k[g] = 0.0;
    if (btw_kind) btw_kind[g] = ABS_NONE;
}
// the kind of up to four slots of one window (vf_engine_set_absolute and vf_engine_set_between on an asynchronous engine)
__global__ void __launch_bounds__(64) k_put_between_kind(int* btw_kind, BtwKindArg a) {
    const int i = threadIdx.x;
    if (i < a.n) btw_kind[a.g[i]] = a.kind[i];
}
__global__ void __launch_bounds__(64) k_read_result(View v, int window, int slot, int which, int* sticky, SolveResult* out) {
    const int t = threadIdx.x;
    const int b = v.sel[window] ^ which;
    if (t < 16) out->state[t] = XS(b, t, (long)window * v.M + slot);
    if (t == 16) { out->cost = v.cost[window]; out->n_acc = v.n_acc[window]; out->n_rej = v.n_rej[window]; out->n_fail = v.n_fail[window]; }
    if (t == 17) { out->sticky[0] = sticky[0]; out->sticky[1] = sticky[1]; sticky[0] = 0; sticky[1] = 0; }
    if (t == 18) out->pad = v.stop_on ? v.done[window] : 0;       // (has the termination rule finished the window?)
}
void launch_set_range(const View& v, int window, int lo, int hi, hipStream_t s) {
    hipLaunchKernelGGL(k_set_range, dim3(1), dim3(1), 0, s, v, window, lo, hi);
}
void launch_bump_lo(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_bump_lo, dim3(nblk(v.B, 64)), dim3(64), 0, s, v);
}
void launch_put_between(const View& v, long g, int a, const BtwArg& rec, hipStream_t s) {
    hipLaunchKernelGGL(k_put_between, dim3(1), dim3(64), 0, s, v, g, a, rec);
}
void launch_put_between_loss(const View& v, const BtwLossArg& a, hipStream_t s) {
    hipLaunchKernelGGL(k_put_between_loss, dim3(1), dim3(64), 0, s, v, a);
}
void launch_reset_tail_loss(const View& v, int* btw_kind, hipStream_t s) {
    hipLaunchKernelGGL(k_reset_tail_loss, dim3(nblk(v.B, 64)), dim3(64), 0, s, v, btw_kind);
}
void launch_put_between_kind(int* btw_kind, const BtwKindArg& a, hipStream_t s) {
    hipLaunchKernelGGL(k_put_between_kind, dim3(1), dim3(64), 0, s, btw_kind, a);
}
void launch_read_result(const View& v, int window, int slot, int which, int* sticky, SolveResult* out, hipStream_t s) {
    hipLaunchKernelGGL(k_read_result, dim3(1), dim3(64), 0, s, v, window, slot, which, sticky, out);
}
void launch_inc_begin(const View& v, double threshold, int appended, int invalid, hipStream_t s) {
    hipLaunchKernelGGL(k_inc_begin, dim3((unsigned)nblk(v.M, 256), (unsigned)v.B), dim3(256), 0, s, v, threshold, appended, invalid);
}
void launch_inc_solve(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_inc_forward, dim3(v.B), dim3(64), 0, s, v);
    hipLaunchKernelGGL(k_inc_backward, dim3(v.B), dim3(64), 0, s, v);
}
void launch_inc_retract(const View& v, hipStream_t s) {
    hipLaunchKernelGGL(k_inc_retract, dim3((unsigned)nblk(v.M, 256), (unsigned)v.B), dim3(256), 0, s, v);
}
void launch_slide(const View& v, const double* sigma15_dev, int reanchor, hipStream_t s) {
    hipLaunchKernelGGL(k_slide, dim3(nblk(v.B, 64)), dim3(64), 0, s, v, sigma15_dev, reanchor);
}
void launch_marginalize_ahead(const View& v, int* status, double* stash, hipStream_t s) {
    hipLaunchKernelGGL(k_marginalize<0>, dim3(v.B), dim3(256), 0, s, v, status, stash);
}
void launch_marg_commit(const View& v, const double* stash, hipStream_t s) {
    hipLaunchKernelGGL(k_marg_commit, dim3(v.B), dim3(256), 0, s, v, stash);
}
void launch_marginalize(const View& v, int slots, int* status, hipStream_t s) {
    // (an engine without far capacity holds no slots and never has far_big set)
    if (v.x_max == 0) hipLaunchKernelGGL(k_marginalize<0>, dim3(v.B), dim3(256), 0, s, v, status, (double*)nullptr);
    else if (far_big_form(v, slots)) hipLaunchKernelGGL(k_marginalize<2>, dim3(v.B), dim3(1024), 0, s, v, status, (double*)nullptr);
    else hipLaunchKernelGGL(k_marginalize<1>, dim3(v.B), dim3(256), 0, s, v, status, (double*)nullptr);
}
void launch_shift_copy(const double* src, double* dst, long n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_shift_copy, dim3(nblk(n, 256)), dim3(256), 0, s, src, dst, n);
}
void launch_shift_btw_a(int* a, long G, int M, int shift, hipStream_t s) {
    hipLaunchKernelGGL(k_shift_btw_a, dim3(nblk(G, 256)), dim3(256), 0, s, a, G, M, shift);
}
void launch_scatter(const double* aos, double* aosoa, long g0, long n, int nf, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_scatter, dim3(nblk(n * nf, 256)), dim3(256), 0, s, aos, aosoa, g0, n, nf);
}
void launch_fixed_jwords(const View& v, long g0, long n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_fixed_jwords, dim3(nblk(n * JS_NJF, 256)), dim3(256), 0, s, v, g0, n);
}
void launch_gather(const double* aosoa, double* aos, long g0, long n, int nf, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_gather, dim3(nblk(n * nf, 256)), dim3(256), 0, s, aosoa, aos, g0, n, nf);
}
void launch_gather_imu_lin(const View& v, int b, long g0, long n, double* aos, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_gather_imu_lin, dim3(nblk(n * IMU_OUT, 256)), dim3(256), 0, s, v, b, g0, n, aos);
}
void launch_scatter_states(const double* aos, double* x, long G, int buf, long g0, long n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_scatter_states, dim3(nblk(n * 16, 256)), dim3(256), 0, s, aos, x, G, buf, g0, n);
}
void launch_gather_states(const double* x, double* aos, long G, const int* sel, int M, int which, long g0, long n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_gather_states, dim3(nblk(n * 16, 256)), dim3(256), 0, s, x, aos, G, sel, M, which, g0, n);
}
