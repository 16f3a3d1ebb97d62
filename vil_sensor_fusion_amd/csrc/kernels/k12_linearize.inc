// kernels/k12_linearize.inc -- K1 / K2: CombinedImuFactor and BetweenFactor<Pose3> residuals + whitened Jacobians (the J stream).
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ K1
// Algorithmic traffic per factor: 222 doubles in (2 states x 16, record 190); out 15 (r) + 202 (101 pairs of J: the 90 words of
// J that do not depend on the states are in the stream since the record was written, write_fixed_jwords) = 3 512 B with the input.
constexpr int K1_BLOCK = 256, K1_WAVES = 1;     // launch bounds of the linearisation kernels: threads per block, waves per execution unit
VF_DI const double* jtile_ptr(const double* base, long gk) { return base + (size_t)(gk >> JT_LOG) * JT_STRIDE; }
// entry (row, col) of the Jacobian of the factor in slot gk of a J stream buffer (0 for a structural zero)
VF_DI double jstream_entry(const double* jbuf, long gk, int row, int col) {
    const int e = JMD.idx[row * 30 + col];
    if (e < 0) return 0.0;
    const int pair = (jcol_is_j(col) ? JS_PI : 0) + (e >> 1);
    return jbuf[(size_t)(gk >> JT_LOG) * JT_STRIDE + ((size_t)pair * JT + (gk & (JT - 1))) * 2 + (e & 1)];
}

// Where a factor's (r | J) goes.  K1: r into the AoSoA residual array, J into the factor's slot of its J-stream tile as
// 16-byte non-temporal stores of two consecutive entries (write-once streams far beyond L2 / MALL: +15 % measured for
// non-temporal): the 74 pairs of the i side and the first 27 = JS_NJV / 2 of the j side -- the 45 pairs behind them are the
// record's, not the states' (vf_jstream.hpp), and are not K1's to write.  (A copy of the i-side pairs of a tile's first
// factor into the tile in front of it, so that K3 would find its halo factor in its own block, cost K1 0.48 ms: 16-byte
// partial-line writes.  K3 reads the halo where it is.)
// `jac` = false (time-sharded windows, factors this rank does not assemble): residual only.
struct HbmSink {
    // The 9x6 bias Jacobians of the record are used twice (bias-corrected delta, bias columns of J) and the second read
    // misses L2 (18 % excess fetch traffic in the PMC counters).  Keeping them in registers (352 -> 406) removed that
    // traffic (2.15 -> 1.71 GB read per launch) and made K1 SLOWER, 0.80 -> 0.855 ms: with one wave per SIMD the kernel is
    // paced by how early its first compute can start, not by its byte count.  Measured, not kept:
    // the core reads them where it uses them, IN(16 + i).
    double* out_r;      // imu_r row of this factor (+ a * TILE)
    double* slot;       // imu_j: tile base + 2 * slot
    bool jac;
    double pend[2];
    VF_DI void r(int a, double x) { __builtin_nontemporal_store(x, out_r + (size_t)a * TILE); }
    VF_DI void pair(int side, int p, double x0, double x1) {
        if (!jac) return;
        d2_t t;
        t.x = x0;
        t.y = x1;
        __builtin_nontemporal_store(t, (d2_t*)(slot + (size_t)((side ? JS_PI : 0) + p) * (JT * 2)));
    }
    VF_DI void j(int row, int col, double x) {
        const int e = JM.idx[row * 30 + col];          // compile-time constants once the core's loops are unrolled
        const int side = jcol_is_j(col) ? 1 : 0;
        if (e & 1) pair(side, e >> 1, pend[side], x);
        else if (e == JM.n[side] - 1) pair(side, e >> 1, x, 0.0);   // odd count: the last entry goes with a zero
        else pend[side] = x;
    }
};
// LDS image of one IMU linearisation = its words of the J stream as they are ([0, 2 JS_PAIRS): i-side pairs then j-side
// pairs), then r (15) and a zero cell the MFMA operand maps point at for structural zeros and padding
constexpr int LJ_R = 2 * JS_PAIRS, LJ_ZERO = LJ_R + 15;
constexpr int LJS = 310;        // LDS stride of one factor (even: the staging writes are 16-byte; 620 dwords = 12 mod 32 banks: the 8 slots of a pair hit 8 different bank groups)
// CombinedImuFactor: residual and whitened 15x30 Jacobian of the factor in slot gk, at the states of buffer b.
__device__ __forceinline__ void linearize_imu_core(const View& v, const int b, const long gk, HbmSink& sink) {
    const double* __restrict__ in = v.imu_in + (size_t)(gk >> 6) * IMU_IN * TILE + (gk & 63);
#define IN(f) in[(size_t)(f) * TILE]
    // the square-root information (120 of the 222 input words, read once) non-temporal: more of the bias Jacobians, which
    // are read twice, survive in L2 until their second use (PMC: 2.15 -> 2.00 GB read per launch; time unchanged)
#define INR(f) __builtin_nontemporal_load(in + (size_t)(f) * TILE)
    struct RRef { HbmSink& s; int a; VF_DI void operator=(double x) const { s.r(a, x); } };
    struct JRef { HbmSink& s; int row, col; VF_DI void operator=(double x) const { s.j(row, col, x); } };
#define OUT(f) (RRef{sink, (f)})
#define JOUT(r, c) (JRef{sink, (r), (c)})

    const State si = load_state(v, b, gk - 1), sj = load_state(v, b, gk);
    // bias-corrected preintegrated delta, NavState::correctPIM, NavState::retract -> predicted state j
    const ImuPrediction p = imu_predict(v, si, ImuRecordHbm{in});
    const double dt = p.dt;
    const V3 tht = p.tht, pt = p.pt, vt = p.vt;
    const M3 Ri = p.Ri, Rj = qrot(sj.q);
    const Q4 eq = p.eq;
    const Q4 qp = qmul(si.q, eq);
    const V3 pp = si.t + mul(Ri, p.xp);
    const V3 vp = si.vel + mul(Ri, p.xv);
    // NavState::localCoordinates(state_j, predicted)
    const V3 rth = qlog(qmul(qconj(sj.q), qp));
    const V3 rp = mulT(Rj, pp - sj.t);
    const V3 rv = mulT(Rj, vp - sj.vel);
    const V3 rba = si.ba - sj.ba, rbg = si.bg - sj.bg;

    // closed-form 3x3 blocks of the unwhitened Jacobian (derivation: DESIGN.md "K1")
    const M3 L = so3_jr_inv(rth);
    const M3 Em = qrot(eq);
    const M3 M1 = mulBT(L, Em);            // d r_theta / d theta_i = L E^T
    const M3 Rji = mulTA(Rj, Ri);          // R_j^T R_i
    const M3 P1 = mulSkew(Rji, neg(pt));   // -R_ji [p~]x
    const M3 V1 = mulSkew(Rji, neg(vt));   // -R_ji [v~]x
    const M3 M5 = mul(L, so3_jr(tht));     // L J_r(theta~)

    // R11 = R[0:9,0:9] stays in registers; R12 / R22 columns are streamed for the bias columns
    double R[45];
#pragma unroll
    for (int a = 0; a < 9; a++)
#pragma unroll
        for (int c = a; c < 9; c++) R[idx9(a, c)] = INR(70 + off15(a) + (c - a));

    double u[9], o[9], rw[15];
    {
        const double r9[9] = {rth.x, rth.y, rth.z, rp.x, rp.y, rp.z, rv.x, rv.y, rv.z};
        double t9[9];
        white9<0, 9>(R, r9, t9);
#pragma unroll
        for (int a = 0; a < 9; a++) rw[a] = t9[a];
#pragma unroll
        for (int a = 9; a < 15; a++) rw[a] = 0.0;
    }

    // columns 0..17: X_i(theta,p) V_i X_j(theta,p) V_j ; rows 9..14 are structurally zero
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // X_i.theta
#pragma unroll
        for (int r = 0; r < 3; r++) { u[r] = col3(M1, r, c); u[3 + r] = col3(P1, r, c); u[6 + r] = col3(V1, r, c); }
        white9<0, 9>(R, u, o);
#pragma unroll
        for (int a = 0; a < 9; a++) JOUT(a, c) = o[a];
        // X_i.p : rows p = R_ji
#pragma unroll
        for (int r = 0; r < 3; r++) { u[r] = 0; u[3 + r] = col3(Rji, r, c); u[6 + r] = 0; }
        white9<3, 6>(R, u, o);
#pragma unroll
        for (int a = 0; a < 6; a++) JOUT(a, 3 + c) = o[a];       // rows 6..8: structural zeros, never written
        // V_i : rows p = dt R_j^T, rows v = R_j^T
#pragma unroll
        for (int r = 0; r < 3; r++) { u[r] = 0; u[3 + r] = dt * Rj.a[c * 3 + r]; u[6 + r] = Rj.a[c * 3 + r]; }
        white9<3, 9>(R, u, o);
#pragma unroll
        for (int a = 0; a < 9; a++) JOUT(a, 6 + c) = o[a];
        // X_j.theta : rows theta = -L^T, p = [rp]x, v = [rv]x
        {
            const M3 Sp = skew(rp), Sv = skew(rv);
#pragma unroll
            for (int r = 0; r < 3; r++) { u[r] = -L.a[c * 3 + r]; u[3 + r] = col3(Sp, r, c); u[6 + r] = col3(Sv, r, c); }
        }
        white9<0, 9>(R, u, o);
#pragma unroll
        for (int a = 0; a < 9; a++) JOUT(a, 9 + c) = o[a];
        // X_j.p : rows p = -I  => -R11(:, 3+c): fixed words of the record, in the stream since the record was written
        // V_j : rows v = -R_j^T
#pragma unroll
        for (int r = 0; r < 3; r++) { u[r] = 0; u[3 + r] = 0; u[6 + r] = -Rj.a[c * 3 + r]; }
        white9<6, 9>(R, u, o);
#pragma unroll
        for (int a = 0; a < 9; a++) JOUT(a, 15 + c) = o[a];
    }
    // Structural zeros of the whitened Jacobian are NOT written: rows 9..14 of the columns 0..17, rows 6..8 of X_i.p,
    // the rows below the diagonal of X_j.p and rows >= 10 + c of the bias columns -- 159 of the 450 entries.  The
    // output buffers are zero-filled when the engine is created and nothing else writes those words, so readers
    // (K3, the read-backs) see zeros; a third of the J write traffic is gone.

    // bias columns: B_i (18..23) and B_j (24..29)
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const int n_rc = 10 + c;  // rows 0..9+c of R(:, 9+c) are nonzero
        double Rc[15];
#pragma unroll
        for (int a = 0; a < 15; a++) Rc[a] = (a < n_rc) ? INR(70 + off15(a) + (9 + c - a)) : 0.0;
        const V3 hth = v3(IN(16 + 0 * 6 + c), IN(16 + 1 * 6 + c), IN(16 + 2 * 6 + c));
        const V3 hp = v3(IN(16 + 3 * 6 + c), IN(16 + 4 * 6 + c), IN(16 + 5 * 6 + c));
        const V3 hv = v3(IN(16 + 6 * 6 + c), IN(16 + 7 * 6 + c), IN(16 + 8 * 6 + c));
        const V3 u0 = mul(M5, hth), u1 = mul(Rji, hp), u2 = mul(Rji, hv);
        u[0] = u0.x; u[1] = u0.y; u[2] = u0.z; u[3] = u1.x; u[4] = u1.y; u[5] = u1.z; u[6] = u2.x; u[7] = u2.y; u[8] = u2.z;
        white9<0, 9>(R, u, o);
        const double rb = (c < 3) ? vget(rba, c) : vget(rbg, c - 3);
#pragma unroll
        for (int a = 0; a < 15; a++) {
            const double bi = (a < 9) ? o[a] + Rc[a] : Rc[a];
            if (a < n_rc) {                       // rows >= 10 + c: structural zeros
                JOUT(a, 18 + c) = bi;                     // (B_j = -Rc: fixed words, like X_j.p)
            }
            rw[a] = fma(Rc[a], rb, rw[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 15; a++) OUT(a) = rw[a];
#undef IN
#undef INR
#undef OUT
#undef JOUT
}

// K1 proper.  SH (time-sharded windows): every rank evaluates the residual of EVERY factor -- the cost of a trial is then
// known on every rank without an exchange -- but writes the Jacobian only of the factors that feed the rows of H it assembles.
template <bool SH>
__device__ __forceinline__ void linearize_imu_factor(const View& v, int which, const long gk) {
    if (gk >= v.G) return;
    const int w = (int)(gk / v.M), k = (int)(gk - (long)w * v.M);
    // (the window's scalars are requested together, in front of the first branch: one memory round trip instead of one
    // per test -- with one wave per SIMD nothing else hides them)
    const int w_lo = v.lo[w], w_hi = v.hi[w], w_sel = v.sel[w], w_done = v.stop_on ? v.done[w] : 0;
    if (k <= w_lo || k >= w_hi || w_done) return;
    if (v.relin_only && !v.relin[w]) return;
    if (v.inc_on && k < v.inc_k[w]) return;      // incremental update: both keyframes of the factor are where they were
    const bool jac = !SH || !shard_skips_factor(v, w, k);
    const int b = w_sel ^ which;
    double* jbuf = v.imu_j + (size_t)b * (size_t)(v.G >> JT_LOG) * JT_STRIDE;
    HbmSink sink;
    sink.out_r = v.imu_r + ((size_t)b * (size_t)(v.G >> 6) + (size_t)(gk >> 6)) * IMU_R * TILE + (gk & 63);
    sink.slot = jbuf + (size_t)(gk >> JT_LOG) * JT_STRIDE + (gk & (JT - 1)) * 2;
    sink.jac = jac;
    linearize_imu_core(v, b, gk, sink);
}

// ------------------------------------------------------------------------------------ K2
// Algorithmic traffic per factor: 42 doubles in (2 poses x 7, record 28), 78 out.
__global__ void __launch_bounds__(K1_BLOCK, K1_WAVES) k_linearize_imu(View v, int which) {
    linearize_imu_factor<false>(v, which, (long)blockIdx.x * K1_BLOCK + threadIdx.x);
}

// BetweenFactor<Pose3> on values: the poses (qa, ta) -> (qb, tb), the record's 28 words answered by rec(f) (measured pose 7, square-root
// information 21).  The whitened residual goes to sink.r(row, x), the whitened Jacobians to sink.ja / sink.jb(row * 6 + col, x), in the
// order K2 has always stored them; the unwhitened residual [rot, trans] is returned.  K2 calls it on the window's states
// (between_core); k_gate_between (kernels/kgate.inc) with a predicted pose in registers.
template <class Rec, class Sink>
__device__ __forceinline__ Xi6 between_values(const Q4 qa, const V3 ta, const Q4 qb, const V3 tb, const Rec& rec, Sink& sink) {
    const Q4 qm = q4(rec(0), rec(1), rec(2), rec(3));
    const V3 tm = v3(rec(4), rec(5), rec(6));

    // hx = T_a^-1 T_b ; err = measured^-1 hx ; r = Logmap(err)
    const M3 Ra = qrot(qa), Rm = qrot(qm);
    const Q4 qh = qmul(qconj(qa), qb);
    const V3 th = mulT(Ra, tb - ta);
    const Q4 qe = qmul(qconj(qm), qh);
    const V3 te = mulT(Rm, th - tm);
    const Xi6 xi = se3_log(qe, te);
    M3 Jw, Q2;
    se3_jr_inv(xi, &Jw, &Q2);
    // Jb = Hlocal ; Ja = -Hlocal Ad(hx^-1) = -[[JR, 0], [Q2 Rh^T - JR [th]x, JR]], JR = Jw Rh^T
    const M3 Rh = qrot(qh);
    const M3 JR = mulBT(Jw, Rh);
    const M3 QR = mulBT(Q2, Rh);
    const M3 JRS = mulSkew(JR, th);

    double Rw[21];
#pragma unroll
    for (int i = 0; i < 21; i++) Rw[i] = rec(7 + i);
    const double ru[6] = {xi.w.x, xi.w.y, xi.w.z, xi.u.x, xi.u.y, xi.u.z};
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double s = 0.0;
#pragma unroll
        for (int c = r; c < 6; c++) s = fma(Rw[off6(r) + c - r], ru[c], s);
        sink.r(r, s);
    }
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double ua[6], ub[6];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            if (c < 3) {
                ua[r] = -col3(JR, r, c);
                ua[3 + r] = -(col3(QR, r, c) - col3(JRS, r, c));
                ub[r] = col3(Jw, r, c);
                ub[3 + r] = col3(Q2, r, c);
            } else {
                ua[r] = 0.0;
                ua[3 + r] = -col3(JR, r, c - 3);
                ub[r] = 0.0;
                ub[3 + r] = col3(Jw, r, c - 3);
            }
        }
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double sa = 0.0, sb = 0.0;
#pragma unroll
            for (int l = r; l < 6; l++) {
                sa = fma(Rw[off6(r) + l - r], ua[l], sa);
                sb = fma(Rw[off6(r) + l - r], ub[l], sb);
            }
            sink.ja(r * 6 + c, sa);
            sink.jb(r * 6 + c, sb);
        }
    }
    return xi;
}

// ... between the keyframes in slots ga -> gk at the states of buffer b (the loads): whitened residual (6) and
// Jacobians (Ja 36, Jb 36) written to out[f * ostride], record read from in[f * istride].  `jac` = false: residual only.
template <bool SH>
__device__ __forceinline__ void between_core(const View& v, const int b, const long ga, const long gk,
                                             const double* __restrict__ in, const size_t istride,
                                             double* __restrict__ out, const size_t ostride, const bool jac) {
    struct Rec {
        const double* __restrict__ in;
        size_t istride;
        VF_DI double operator()(int f) const { return in[(size_t)f * istride]; }
    };
    struct Sink {
        double* __restrict__ out;
        size_t ostride;
        bool jac;
        VF_DI void r(int f, double x) { __builtin_nontemporal_store(x, out + (size_t)f * ostride); }
        VF_DI void j(int f, double x) { if (!SH || jac) __builtin_nontemporal_store(x, out + (size_t)f * ostride); }
        VF_DI void ja(int e, double x) { j(6 + e, x); }
        VF_DI void jb(int e, double x) { j(42 + e, x); }
    };
    const Q4 qa = q4(XS(b, 0, ga), XS(b, 1, ga), XS(b, 2, ga), XS(b, 3, ga));
    const V3 ta = v3(XS(b, 4, ga), XS(b, 5, ga), XS(b, 6, ga));
    const Q4 qb = q4(XS(b, 0, gk), XS(b, 1, gk), XS(b, 2, gk), XS(b, 3, gk));
    const V3 tb = v3(XS(b, 4, gk), XS(b, 5, gk), XS(b, 6, gk));
    Sink sink{out, ostride, jac};
    between_values(qa, ta, qb, tb, Rec{in, istride}, sink);
}

// Robust loss on a band between factor (View::btw_loss; DESIGN.md "4i"): the factor in its square-root form, an ordinary least-squares
// factor with residual r^ = alpha(s) r, s = |r|, and Jacobian J^ = (alpha I + gamma r r^T) J (vf_robust.hpp), written where r and J
// are written -- 0.5 |r^|^2 = rho(s) and J^^T r^ = (rho' / s) J^T r, so nothing that reads btw_out knows about losses.
// It is applied BEHIND between_core, to the 78 words the lane has just stored, and not in a sink of between_values: a sink that
// keeps r and a column in registers changes how the compiler contracts the multiply-adds in front of it (measured: the last
// residual row and the translation rows of J of a slot WITHOUT a loss came out an ulp off the kernels that know no losses).  This
// way the words of a slot without a loss, and of a Huber inlier (s <= k, s = k included), are those kernels' code and bits, and
// only a factor the loss changes pays the second pass: r (6), then column by column the 6 + 6 entries of Ja / Jb and their dots
// r^T Ja[:, c], r^T Jb[:, c] -- read back from the lane's own words (same lane, same addresses: program order).
// STRIDE: doubles between two of the 78 words -- TILE in btw_out (the band kernels, which name none), 1 in x_out (k_linearize_extra).
template <int STRIDE = TILE>
__device__ __forceinline__ void robustify_between(double* out, const int loss, const double k) {
    asm volatile("" ::: "memory");            // (the words are read back, not kept in 78 registers across between_core)
    double rr[6];
    double s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) { rr[i] = out[(size_t)i * STRIDE]; s2 = fma(rr[i], rr[i], s2); }
    const double s = sqrt(s2);
    if (loss == LOSS_HUBER && s <= k) return;       // (a NaN norm is no inlier: alpha is NaN and so is every word below)
    const double alpha = robust_alpha(loss, s, k), gamma = robust_gamma(loss, s, k);
#pragma unroll
    for (int i = 0; i < 6; i++) __builtin_nontemporal_store(alpha * rr[i], out + (size_t)i * STRIDE);
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double pa[6], pb[6], da = 0.0, db = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            pa[i] = out[(size_t)(6 + i * 6 + c) * STRIDE];
            pb[i] = out[(size_t)(42 + i * 6 + c) * STRIDE];
            da = fma(rr[i], pa[i], da);
            db = fma(rr[i], pb[i], db);
        }
        da *= gamma;
        db *= gamma;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            __builtin_nontemporal_store(fma(da, rr[i], alpha * pa[i]), out + (size_t)(6 + i * 6 + c) * STRIDE);
            __builtin_nontemporal_store(fma(db, rr[i], alpha * pb[i]), out + (size_t)(42 + i * 6 + c) * STRIDE);
        }
    }
}

// Absolute factors in the between slot (vf_engine_set_absolute; DESIGN.md "4k"): a factor on keyframe gk ALONE, written into gk's
// own slot as a between factor from gk - 1 whose first Jacobian is 36 exact zeros -- J^T J then has J_u^T J_u on block (gk, gk) and
// exact zeros on the blocks of gk - 1, J^T r has J_u^T r_u on gk, the cost 0.5 |r_u|^2: a unary factor's, and nothing that reads
// btw_out knows the difference.  The slot's kind (ABS_*) is an array of the engine's, an ARGUMENT of the kernels that read it.
//
// ABS_NONE and ABS_POSE: the between factor, and GTSAM's PriorFactor<Pose3> -- r = R Log(Z^-1 T_b), J_u = R J_r^-1(Log(Z^-1 T_b)),
// which is between_values with (qa, ta) = (identity, 0): Ra = I, qh = qb and th = tb come out exactly, and its jb is this Hlocal.
// ONE call serves both, so that a wave that holds both kinds runs it once: `unary` picks the first pose, and the sink's ja
// stores 0.0 whatever it is handed.
__device__ __forceinline__ void between_or_pose_core(const View& v, const int b, const long ga, const long gk, const bool unary,
                                                     const double* __restrict__ in, double* __restrict__ out) {
    struct Rec {
        const double* __restrict__ in;
        VF_DI double operator()(int f) const { return in[(size_t)f * TILE]; }
    };
    struct Sink {
        double* __restrict__ out;
        bool unary;
        VF_DI void r(int f, double x) { __builtin_nontemporal_store(x, out + (size_t)f * TILE); }
        VF_DI void ja(int e, double x) { __builtin_nontemporal_store(unary ? 0.0 : x, out + (size_t)(6 + e) * TILE); }
        VF_DI void jb(int e, double x) { __builtin_nontemporal_store(x, out + (size_t)(42 + e) * TILE); }
    };
    // (slot ga = gk - 1 of a unary factor is inside the window: its state is loaded like any other and not used)
    const Q4 qs = q4(XS(b, 0, ga), XS(b, 1, ga), XS(b, 2, ga), XS(b, 3, ga));
    const V3 ts = v3(XS(b, 4, ga), XS(b, 5, ga), XS(b, 6, ga));
    const Q4 qa = unary ? q4(1.0, 0.0, 0.0, 0.0) : qs;
    const V3 ta = unary ? v3(0.0, 0.0, 0.0) : ts;
    const Q4 qb = q4(XS(b, 0, gk), XS(b, 1, gk), XS(b, 2, gk), XS(b, 3, gk));
    const V3 tb = v3(XS(b, 4, gk), XS(b, 5, gk), XS(b, 6, gk));
    Sink sink{out, unary};
    between_values(qa, ta, qb, tb, Rec{in}, sink);
}

// ABS_POSITION: GTSAM's GPSFactor.  e = t_b - z in the world frame, r = R3 e, J_u = R3 [0 | R_b] (k_retract moves t by R_b dp, and
// the rotation has no first-order effect on t).  The record is [1, 0, 0, 0, z, R] with only the translation block of R's 21 words
// in use: R3 is rows 3..5 of the upper triangle, and rows 3..5 of the slot carry the factor, as the translation rows of a pose do
// (ABS_POSITION_ROW0); rows 0..2 of r, Ja and Jb, all of Ja and the rotation columns of Jb are exact zeros.
__device__ __forceinline__ void absolute_position_core(const View& v, const int b, const long gk, const double* __restrict__ in,
                                                       double* __restrict__ out) {
    const Q4 qb = q4(XS(b, 0, gk), XS(b, 1, gk), XS(b, 2, gk), XS(b, 3, gk));
    const V3 e = v3(XS(b, 4, gk), XS(b, 5, gk), XS(b, 6, gk)) - v3(in[4 * TILE], in[5 * TILE], in[6 * TILE]);
    M3 R3;      // (upper triangular: the three words below the diagonal stay zero)
    R3.a[0] = in[(size_t)(7 + off6(3)) * TILE]; R3.a[1] = in[(size_t)(7 + off6(3) + 1) * TILE]; R3.a[2] = in[(size_t)(7 + off6(3) + 2) * TILE];
    R3.a[3] = 0.0;                              R3.a[4] = in[(size_t)(7 + off6(4)) * TILE];     R3.a[5] = in[(size_t)(7 + off6(4) + 1) * TILE];
    R3.a[6] = 0.0;                              R3.a[7] = 0.0;                                  R3.a[8] = in[(size_t)(7 + off6(5)) * TILE];
    const M3 Rb = qrot(qb);
    const double ev[3] = {e.x, e.y, e.z};
    static_assert(ABS_POSITION_ROW0 == 3, "rows 3..5 of the slot");
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = 0.0;
#pragma unroll
        for (int c = i; c < 3; c++) s = fma(R3.a[i * 3 + c], ev[c], s);
        __builtin_nontemporal_store(0.0, out + (size_t)i * TILE);
        __builtin_nontemporal_store(s, out + (size_t)(ABS_POSITION_ROW0 + i) * TILE);
    }
#pragma unroll
    for (int e36 = 0; e36 < 36; e36++) __builtin_nontemporal_store(0.0, out + (size_t)(6 + e36) * TILE);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double s = 0.0;
            if (c >= 3) {
#pragma unroll
                for (int l = i; l < 3; l++) s = fma(R3.a[i * 3 + l], Rb.a[l * 3 + c - 3], s);
            }
            __builtin_nontemporal_store(0.0, out + (size_t)(42 + i * 6 + c) * TILE);
            __builtin_nontemporal_store(s, out + (size_t)(42 + (ABS_POSITION_ROW0 + i) * 6 + c) * TILE);
        }
}

// RB: the engine holds losses (View::btw_loss is not null; never on a time-sharded engine).  The kernels without them are the
// RB = false instances, which read neither array: what they were before losses existed.
// AB: the engine holds absolute factors too (btw_kind, the slots' kinds: made behind the loss arrays, so AB implies RB).  The
// instances without them read no kind and are what they were before absolute factors existed.
template <bool SH, bool RB = false, bool AB = false>
__device__ __forceinline__ void linearize_between_factor(const View& v, int which, const long gk, const int* __restrict__ btw_kind = nullptr) {
    static_assert(!(SH && RB), "losses on time-sharded windows are not built");
    static_assert(!AB || RB, "the kinds come behind the loss arrays");
    if (gk >= v.G) return;
    const int w = (int)(gk / v.M), k = (int)(gk - (long)w * v.M);
    const int lo = v.lo[w], w_hi = v.hi[w], w_sel = v.sel[w], w_done = v.stop_on ? v.done[w] : 0;
    const int a = v.btw_a[gk];                 // (all five requested together: one round trip)
    int loss = LOSS_NONE;
    double loss_k = 0.0;
    int kind = ABS_NONE;
    if (RB) { loss = v.btw_loss[gk]; loss_k = v.btw_loss_k[gk]; }
    if (AB) kind = btw_kind[gk];               // (... and the kind with them)
    if (k <= lo || k >= w_hi || w_done) return;
    if (v.relin_only && !v.relin[w]) return;
    if (v.inc_on && k < v.inc_k[w]) return;
    const bool jac = !SH || !shard_skips_factor(v, w, k);
    if (a < lo || a >= k) return;
    const int b = w_sel ^ which;
    const double* __restrict__ in = v.btw_in + (size_t)(gk >> 6) * BTW_IN * TILE + (gk & 63);
    double* __restrict__ out = v.btw_out + ((size_t)b * (size_t)(v.G >> 6) + (size_t)(gk >> 6)) * BTW_OUT * TILE + (gk & 63);
    if (AB) {
        if (kind == ABS_POSITION) absolute_position_core(v, b, gk, in, out);
        else between_or_pose_core(v, b, (long)w * v.M + a, gk, kind == ABS_POSE, in, out);
    } else between_core<SH>(v, b, (long)w * v.M + a, gk, in, TILE, out, TILE, jac);
    if (RB && loss != LOSS_NONE) robustify_between(out, loss, loss_k);
}
