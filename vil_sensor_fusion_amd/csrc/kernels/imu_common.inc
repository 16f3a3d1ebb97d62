// kernels/imu_common.inc -- the IMU arithmetic that more than one kernel needs, once: the prediction of keyframe j from keyframe i
// (K1, k_predict, k_slide, k_propagate) and pick9.
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ pick9
// entry k of a 3 x 3 matrix held in registers, k known only at run time: selects on nine values loaded unconditionally (indexing
// the array, or loading inside the selects' arms, keeps the matrix in scratch: K0's 368 bytes per lane)
VF_DI double pick9(const M3& A, int k) {
    const double a0 = A.a[0], a1 = A.a[1], a2 = A.a[2], a3 = A.a[3], a4 = A.a[4], a5 = A.a[5], a6 = A.a[6], a7 = A.a[7], a8 = A.a[8];
    const double r0 = k == 1 ? a1 : (k == 2 ? a2 : a0);
    const double r1 = k == 4 ? a4 : (k == 5 ? a5 : a3);
    const double r2 = k == 7 ? a7 : (k == 8 ? a8 : a6);
    return k < 3 ? r0 : (k < 6 ? r1 : r2);
}

// ------------------------------------------------------------------------------------ imu_predict
// Keyframe j as the IMU factor predicts it from keyframe i: the bias-corrected preintegrated delta, NavState::correctPIM, and what
// the retraction onto keyframe i needs.  rec(f) answers word f of the IMU record (dt_ij, mean, the bias it was integrated with,
// H) and is asked each time a word is used: it reads, it does not cache (HbmSink's note in k12_linearize.inc says why).
struct ImuPrediction {
    double dt;
    V3 tht, pt, vt;     // bias-corrected delta: d + H (b_i - bhat)   (biasCorrectedDelta)
    M3 Ri;
    V3 xp, xv;          // NavState::correctPIM, in the frame of keyframe i
    Q4 eq;              // qexp(tht)
};
template <class Rec>
VF_DI ImuPrediction imu_predict(const View& v, const State& si, const Rec& rec) {
    ImuPrediction p;
    p.dt = rec(0);
    const V3 dba = si.ba - v3(rec(10), rec(11), rec(12));
    const V3 dbg = si.bg - v3(rec(13), rec(14), rec(15));
    double xt[9];
#pragma unroll
    for (int r = 0; r < 9; r++) {
        double s = rec(1 + r);
        s = fma(rec(16 + r * 6 + 0), dba.x, s);
        s = fma(rec(16 + r * 6 + 1), dba.y, s);
        s = fma(rec(16 + r * 6 + 2), dba.z, s);
        s = fma(rec(16 + r * 6 + 3), dbg.x, s);
        s = fma(rec(16 + r * 6 + 4), dbg.y, s);
        s = fma(rec(16 + r * 6 + 5), dbg.z, s);
        xt[r] = s;
    }
    p.tht = v3(xt[0], xt[1], xt[2]);
    p.pt = v3(xt[3], xt[4], xt[5]);
    p.vt = v3(xt[6], xt[7], xt[8]);
    p.Ri = qrot(si.q);
    const V3 grav = v3(v.grav[0], v.grav[1], v.grav[2]);
    const V3 gib = mulT(p.Ri, grav), vib = mulT(p.Ri, si.vel);
    p.xp = p.pt + p.dt * vib + (0.5 * p.dt * p.dt) * gib;
    p.xv = p.vt + p.dt * gib;
    p.eq = qexp(p.tht);
    return p;
}
// NavState::retract of the prediction onto keyframe i, the biases carried over (PreintegrationBase::predict)
VF_DI State predicted_state(const State& si, const ImuPrediction& p) {
    State o;
    o.q = qnormalize(qmul(si.q, p.eq));
    o.t = si.t + mul(p.Ri, p.xp);
    o.vel = si.vel + mul(p.Ri, p.xv);
    o.ba = si.ba;
    o.bg = si.bg;
    return o;
}
// the accessor over a record of v.imu_in (AoSoA tiles of 64): `in` points at word 0 of the factor's record
struct ImuRecordHbm {
    const double* __restrict__ in;
    VF_DI double operator()(int f) const { return in[(size_t)f * TILE]; }
};

// ------------------------------------------------------------------------------------ fixed words of the J stream
// Word t (0 .. JS_NJF - 1) of the j side's fixed words of the factor in slot gk (vf_jstream.hpp): entry (row, col) of J with col
// in X_j.p (12..14) or B_j (24..29), which is -R(row, col - 9) resp. -R(row, col - 15) of the record's square-root information
// whatever the states are.  Written into BOTH buffers of imu_j -- K1 writes neither -- by whoever writes the record: K0 from the
// R it has just made, k_fixed_jwords from the record where a record arrives by another road (vf_engine_set_imu,
// vf_engine_grow).  One thread per word; sqrt_info(row, col) answers R, row <= col.  The negation is the one K1 made (exact).
template <class SqrtInfo>
VF_DI void write_fixed_jwords(const View& v, const long gk, const int t, const SqrtInfo& sqrt_info) {
    const int e = JS_NJV + t, f = JMD.fld[2 * JS_PI + e];
    const int row = f / 30, col = f - row * 30;
    const double x = -sqrt_info(row, col < 24 ? col - 9 : col - 15);
    const size_t word = (size_t)(gk >> JT_LOG) * JT_STRIDE + ((size_t)(JS_PI + (e >> 1)) * JT + (gk & (JT - 1))) * 2 + (e & 1);
    v.imu_j[word] = x;
    v.imu_j[(size_t)(v.G >> JT_LOG) * JT_STRIDE + word] = x;
}
// ... for the factors in slots [g0, g0 + n), from their records in v.imu_in
__global__ void __launch_bounds__(256) k_fixed_jwords(View v, long g0, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * JS_NJF) return;
    const long gk = g0 + i / JS_NJF;
    const int t = (int)(i % JS_NJF);
    const double* __restrict__ in = v.imu_in + (size_t)(gk >> 6) * IMU_IN * TILE + (gk & 63);
    write_fixed_jwords(v, gk, t, [in](int row, int col) { return in[(size_t)(70 + off15(row) + (col - row)) * TILE]; });
}
