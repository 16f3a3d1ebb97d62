// kernels/k0_preintegrate.inc -- K0: combined-IMU preintegration incl. the 15 x 15 covariance (IMUManager.cpp:27-74 + GTSAM PIM).
// A section of vf_kernels.hip (ONE translation unit: the kernels share device helpers and must inline as they always have);
// included from there, inside namespace vf, never compiled by itself.
// ------------------------------------------------------------------------------------ K0
// IMU preintegration, one 256-thread workgroup per factor: PreintegratedCombinedMeasurements::
// integrateMeasurement over the factor's steps (mean, bias Jacobians, 15x15 covariance; GTSAM 4.0.x tangent
// form), then the noise model R = chol_upper(cov^-1) of the CombinedImuFactor built at
// gtsam_fusion/src/gtsam_fusion/IMUManager.cpp:68-73.  Runs once per factor (not per LM iteration), and so leaves, beside the
// record, the 90 words of the factor's Jacobian that are columns of -R whatever the states (write_fixed_jwords, imu_common.inc).
// F, P and F P live in LDS, thread (i, j) owns entry (i, j) of the 15x15 products; the small 3x3 quantities of a
// step are computed by every thread.  (The first version ran one LANE per factor with the 15x15 work in per-lane
// scratch arrays: 2-4 ms whatever the batch, i.e. most of a GraphManager::solve, which preintegrates one factor.)
// Every entry is accumulated in the same order as a plain triple loop would, so the result does not depend on
// the mapping.
// TAIL = false: factors [g0, g0 + n) of consecutive slots, bias estimates handed in (vf_engine_preintegrate).
// TAIL = true (vf_engine_ingest_tail, the ingest half of a fixed-lag update for ALL windows in one launch): block w
// preintegrates the factor that ends at window w's NEXT keyframe, slot hi[w], with the window's CURRENT bias estimate -- the
// bias of its last keyframe in the current buffer, what GraphManager::reserveNode passes as getBias()
// (GraphManager.cpp:59) -- and stages the between record that ends at the same keyframe (GraphManager.cpp:83-88).
template <bool TAIL>
__global__ void __launch_bounds__(256) k_preintegrate_t(View v, long g0, int n, const int* __restrict__ off,
                                                       const double* __restrict__ steps,
                                                       const double* __restrict__ bhat6, const int* __restrict__ tail_a,
                                                       const double* __restrict__ tail_btw, ImuCov prm, int* status) {
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= n) return;
    __shared__ double sF[225], sP[225], sT[225], sH[54], sHn[54];
    __shared__ int s_ok;
    const int i = tid / 15, j = tid - i * 15;          // entry of the 15x15 matrices (tid < 225)
    const int hi_ = tid / 6, hj = tid - hi_ * 6;       // entry of the 9x6 bias Jacobian (tid < 54)
    long gk = g0 + f;
    double bh[6];
    if (TAIL) {
        const int hi_w = v.hi[f];
        if (hi_w >= v.M || hi_w <= v.lo[f]) {          // no free slot / empty window: reported, nothing written
            if (tid == 0) atomicOr(status, 2);
            return;
        }
        gk = (long)f * v.M + hi_w;
        const int b = v.sel[f];
#pragma unroll
        for (int c = 0; c < 6; c++) bh[c] = XS(b, 10 + c, gk - 1);
    } else {
#pragma unroll
        for (int c = 0; c < 6; c++) bh[c] = bhat6[(size_t)f * 6 + c];
    }
    const V3 bacc = v3(bh[0], bh[1], bh[2]), bgyr = v3(bh[3], bh[4], bh[5]);
    V3 th = v3(0, 0, 0), pos = v3(0, 0, 0), vel = v3(0, 0, 0);
    double dtij = 0.0;
    if (tid < 225) sP[tid] = 0.0;
    if (tid < 54) sH[tid] = 0.0;
    if (tid == 0) s_ok = 1;
    __syncthreads();
    for (int s = off[f]; s < off[f + 1]; s++) {
        const double* st = steps + (size_t)s * 7;
        const double dt = st[0], dt22 = 0.5 * dt * dt;
        const V3 acc = v3(st[1], st[2], st[3]) - bacc, om = v3(st[4], st[5], st[6]) - bgyr;
        const M3 Jr = so3_jr(th), invD = so3_jr_inv(th);
        const V3 wt = mul(invD, om);
        const M3 R = qrot(qexp(th));
        const V3 anav = mul(R, acc);
        const M3 wH = mul(invD, so3_jr_apply_dtheta(th, wt));   // -w_tangent_H_theta
        const M3 aH = mul(mulSkew(R, neg(acc)), Jr);            // a_nav_H_theta
        // F = [[A, Fb], [0, I]]
        if (tid < 225) {
            double x = i == j ? 1.0 : 0.0;
            if (i < 3 && j < 3) x -= wH.a[i * 3 + j] * dt;
            if (i >= 3 && i < 6 && j < 3) x = aH.a[(i - 3) * 3 + j] * dt22;
            if (i >= 6 && i < 9 && j < 3) x = aH.a[(i - 6) * 3 + j] * dt;
            if (i < 3 && j >= 12) x = -invD.a[i * 3 + j - 12] * dt;                 // theta_H_biasOmega = -C.top
            if (i >= 6 && i < 9 && j >= 9 && j < 12) x = -R.a[(i - 6) * 3 + j - 9] * dt;   // vel_H_biasAcc = -B.bottom
            if (i >= 3 && i < 6 && j == i + 3) x = dt;
            sF[tid] = x;
        }
        __syncthreads();
        // bias Jacobians: H <- A H - [B | C]
        if (tid < 54) {
            double a = 0.0;
            for (int l = 0; l < 9; l++) a = fma(sF[hi_ * 15 + l], sH[l * 6 + hj], a);
            if (hi_ >= 3 && hi_ < 6 && hj < 3) a -= R.a[(hi_ - 3) * 3 + hj] * dt22;
            if (hi_ >= 6 && hj < 3) a -= R.a[(hi_ - 6) * 3 + hj] * dt;
            if (hi_ < 3 && hj >= 3) a -= invD.a[hi_ * 3 + hj - 3] * dt;
            sHn[tid] = a;
        }
        // covariance: P <- F P F^T + G Q G^T
        if (tid < 225) {
            double a = 0.0;
            for (int l = 0; l < 15; l++) a = fma(sF[i * 15 + l], sP[l * 15 + j], a);
            sT[tid] = a;
        }
        __syncthreads();
        if (tid < 54) sH[tid] = sHn[tid];
        if (tid < 225) {
            double a = 0.0;
            for (int l = 0; l < 15; l++) a = fma(sT[i * 15 + l], sF[j * 15 + l], a);
            const double sv = (prm.acc + prm.bias_int) * dt, sr = (prm.gyro + prm.bias_int) * dt;
            if (i >= 6 && i < 9 && j >= 6 && j < 9) {           // (1/dt) vHb (aCov+int) vHb^T
                const M3 RRt = mulBT(R, R);
                a += sv * RRt.a[(i - 6) * 3 + j - 6];
            }
            if (i < 3 && j < 3) {                               // (1/dt) tHb (wCov+int) tHb^T
                const M3 DDt = mulBT(invD, invD);
                a += sr * DDt.a[i * 3 + j];
            }
            if (i == j && i >= 3 && i < 6) a += dt * prm.integration;
            if (i == j && i >= 9 && i < 12) a += dt * prm.bias_acc;
            if (i == j && i >= 12) a += dt * prm.bias_omega;
            sP[tid] = a;
        }
        // mean
        th = th + dt * wt;
        pos = pos + dt * vel + dt22 * anav;
        vel = vel + dt * anav;
        dtij += dt;
        __syncthreads();
    }
    // R upper with R^T R = P^-1: reverse Cholesky P = U U^T (U upper, in sF), R = U^-1 (in sT)
    if (tid < 225) { sF[tid] = 0.0; sT[tid] = 0.0; }
    __syncthreads();
    for (int c = 14; c >= 0; c--) {
        if (tid == 0) {
            double d = sP[c * 15 + c];
            for (int l = c + 1; l < 15; l++) d = fma(-sF[c * 15 + l], sF[c * 15 + l], d);
            if (!(d > 0.0)) { s_ok = 0; d = 1.0; }
            sF[c * 15 + c] = sqrt(d);
        }
        __syncthreads();
        if (tid < c) {                                          // row tid of column c
            const double ujj = sF[c * 15 + c];
            double a = 0.5 * (sP[tid * 15 + c] + sP[c * 15 + tid]);
            for (int l = c + 1; l < 15; l++) a = fma(-sF[tid * 15 + l], sF[c * 15 + l], a);
            sF[tid * 15 + c] = a / ujj;
        }
        __syncthreads();
    }
    if (tid < 15) {                                             // column tid of U^-1, bottom up
        const int c = tid;
        sT[c * 15 + c] = 1.0 / sF[c * 15 + c];
        for (int r = c - 1; r >= 0; r--) {
            double a = 0.0;
            for (int l = r + 1; l <= c; l++) a = fma(sF[r * 15 + l], sT[l * 15 + c], a);
            sT[r * 15 + c] = -a / sF[r * 15 + r];
        }
    }
    __syncthreads();
    double* out = v.imu_in + (size_t)(gk >> 6) * IMU_IN * TILE + (gk & 63);
    if (TAIL) {
        if (tid >= 224 && tid < 224 + BTW_IN)
            v.btw_in[((size_t)(gk >> 6) * BTW_IN + (tid - 224)) * TILE + (gk & 63)] = tail_btw[(size_t)f * BTW_IN + tid - 224];
        if (tid == 255) v.btw_a[gk] = tail_a[f];
    }
    if (tid < IMU_IN) {
        double x;
        if (tid == 0) x = dtij;
        else if (tid < 4) x = tid == 1 ? th.x : (tid == 2 ? th.y : th.z);
        else if (tid < 7) x = tid == 4 ? pos.x : (tid == 5 ? pos.y : pos.z);
        else if (tid < 10) x = tid == 7 ? vel.x : (tid == 8 ? vel.y : vel.z);
        else if (tid < 16) x = tid == 10 ? bh[0] : (tid == 11 ? bh[1] : (tid == 12 ? bh[2] : (tid == 13 ? bh[3] : (tid == 14 ? bh[4] : bh[5]))));
        else if (tid < 70) x = sH[tid - 16];
        else {                                                  // packed upper triangle, row-major
            int o = tid - 70, r = 0;
            while (o >= 15 - r) { o -= 15 - r; r++; }
            x = sT[r * 15 + r + o];
        }
        out[(size_t)tid * TILE] = x;
    }
    // ... and the words of the factor's Jacobian that are this R and no state's, into both buffers of the J stream
    if (tid < JS_NJF) {
        const double* T = sT;
        write_fixed_jwords(v, gk, tid, [T](int row, int col) { return T[row * 15 + col]; });
    }
    if (tid == 0 && (!s_ok || off[f + 1] == off[f])) atomicOr(status, 1);
}
