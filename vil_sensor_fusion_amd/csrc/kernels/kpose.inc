// kernels/kpose.inc -- Kpm: the pose marginal of every solved keyframe in the layout of nav_msgs/Odometry, its inverse and the
// keyframe's pose as (x, y, z, roll, pitch, yaw): what the degeneracy metrics (K6, vf_degeneracy.hip) take, left on the device.
// A section of vf_kernels.hip (ONE translation unit); included from there, inside namespace vf, never compiled by itself.
//
// Launched by vf_engine_marginals_ex (VF_MARGINALS_POSE) behind the selected inversion and the far downdate, on the same stream.
// One lane per keyframe, one wave per 64 consecutive keyframes of a window's range [lo, hi):
//     cov   = A Sigma_pp A^T,  A = diag(R, R) P,  P the swap [omega, v] -> [v, omega]      (covariance.ros_pose_covariance)
//     info  = cov^-1 by a 6 x 6 Cholesky in registers (a pivot that is not positive: NaN throughout)
//     pose  = (t, euler angles of R, static x-y-z: tf.transformations.euler_from_quaternion)
// Sigma_pp is the leading 6 x 6 of the keyframe's slot of sig (its first 21 doubles, h_tri order) and R the rotation of the state
// the marginals were linearised at (buffer sel[w]).  Each product is computed as ONE triangle and mirrored, so cov and info are
// symmetric to the bit (K6's condition_number answers NaN for a matrix that is not).  A window whose factorisation failed
// gets NaN in all three.
// Traffic per keyframe: 168 B of a 2 760-B slot + 56 B of state in, 624 B out.  Both sides go through LDS: the 21 doubles of
// 64 slots are fetched by the wave together (lane = word of a slot: 8-byte loads, slots are only 8-byte aligned), and the
// records of a tile, contiguous in HBM, leave as 16-byte stores, fully coalesced (a lane storing its own 288-byte record
// would touch 64 lines per store instruction).  One LDS image of 64 x PM_LD doubles serves the four stages in turn.
constexpr int PM_LD = 37;         // LDS stride of one record (36 + 1 pad: lanes writing entry e of their own record hit distinct banks)
constexpr int PM_IN = 21;         // doubles of a slot that are read (odd: the same holds for the staged input)

// the tile's records (n of them, W doubles each, staged at stride PM_LD) -> dst, 16 bytes per lane and store
template <int W>
VF_DI void pm_flush(const double* __restrict__ img, double* __restrict__ dst, int n, int lane) {
    static_assert(W % 2 == 0, "records are whole 16-byte cells");
    d2_t* __restrict__ out = reinterpret_cast<d2_t*>(dst);
    for (int c = lane; c < n * (W / 2); c += 64) {
        const int r = c / (W / 2), j = 2 * (c - r * (W / 2));
        d2_t x;
        x.x = img[r * PM_LD + j];
        x.y = img[r * PM_LD + j + 1];
        __builtin_nontemporal_store(x, out + c);
    }
}

// C = R S R^T for a symmetric S: the triangle i >= j, mirrored
VF_DI void pm_congruence_sym(const M3& R, const M3& S, double (&c)[36], int o) {
    const M3 T = mul(R, S);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            const double x = fma(T.a[i * 3], R.a[j * 3], fma(T.a[i * 3 + 1], R.a[j * 3 + 1], T.a[i * 3 + 2] * R.a[j * 3 + 2]));
            c[(o + i) * 6 + o + j] = x;
            c[(o + j) * 6 + o + i] = x;
        }
}

__global__ void __launch_bounds__(64) k_pose_marginals(View v, const int* __restrict__ failed, const double* __restrict__ sig,
                                                       double* __restrict__ pm_cov, double* __restrict__ pm_info, double* __restrict__ pm_pose,
                                                       int* __restrict__ pm_range) {
    __shared__ double img[64 * PM_LD];
    const int w = blockIdx.y, lane = threadIdx.x;
    int lo = v.lo[w], hi = v.hi[w];
    if (hi - lo <= 0 || hi > v.M || lo < 0) lo = hi = 0;
    // the range these records are of, for the scores' kernel (the window's own range may move on before it runs)
    if (blockIdx.x == 0 && lane == 0) { pm_range[2 * w] = lo; pm_range[2 * w + 1] = hi; }
    const int base = lo + 64 * (int)blockIdx.x;
    if (base >= hi) return;
    const int n = hi - base < 64 ? hi - base : 64;
    const bool on = lane < n, bad = failed[w] != 0;
    const size_t g0 = (size_t)w * v.M + base;
    const double nan = __builtin_nan("");
    double c[36], q[36], pose[6];
    if (!bad) {
        const double* __restrict__ src = sig + g0 * SIG_SLOT;
        for (int e = lane; e < n * PM_IN; e += 64) {
            const int r = e / PM_IN, j = e - r * PM_IN;
            img[r * PM_IN + j] = __builtin_nontemporal_load(src + (size_t)r * SIG_SLOT + j);
        }
    }
    __syncthreads();
    if (on && !bad) {
        const int b = v.sel[w];
        const long gk = (long)g0 + lane;
        const Q4 qt = q4(XS(b, 0, gk), XS(b, 1, gk), XS(b, 2, gk), XS(b, 3, gk));
        pose[0] = XS(b, 4, gk); pose[1] = XS(b, 5, gk); pose[2] = XS(b, 6, gk);
        const M3 R = qrot(qt);
        const double* __restrict__ s = img + lane * PM_IN;
        M3 Srr, Stt, Str;        // Sigma[omega, omega], Sigma[v, v], Sigma[v, omega]
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Srr.a[i * 3 + j] = s[i >= j ? h_tri(i, j) : h_tri(j, i)];
                Stt.a[i * 3 + j] = s[i >= j ? h_tri(3 + i, 3 + j) : h_tri(3 + j, 3 + i)];
                Str.a[i * 3 + j] = s[h_tri(3 + i, j)];
            }
        pm_congruence_sym(R, Stt, c, 0);
        pm_congruence_sym(R, Srr, c, 3);
        const M3 X = mulBT(mul(R, Str), R);     // cov[t, r]; cov[r, t] is its transpose
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) { c[i * 6 + 3 + j] = X.a[i * 3 + j]; c[(3 + j) * 6 + i] = X.a[i * 3 + j]; }
        // cov = L L^T, Li = L^-1 (lower), info = Li^T Li
        double L[36], Li[36];
        bool spd = true;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double d = c[j * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) d = fma(-L[j * 6 + k], L[j * 6 + k], d);
            if (!(d > 0.0)) spd = false;
            const double ljj = sqrt(d), inv = 1.0 / ljj;
            L[j * 6 + j] = ljj;
            Li[j * 6 + j] = inv;
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double a = c[i * 6 + j];
#pragma unroll
                for (int k = 0; k < j; k++) a = fma(-L[i * 6 + k], L[j * 6 + k], a);
                L[i * 6 + j] = a * inv;
            }
        }
#pragma unroll
        for (int j = 0; j < 6; j++)
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double a = 0.0;
#pragma unroll
                for (int k = j; k < i; k++) a = fma(L[i * 6 + k], Li[k * 6 + j], a);
                Li[i * 6 + j] = -a * Li[i * 6 + i];
            }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double a = 0.0;
#pragma unroll
                for (int k = i; k < 6; k++) a = fma(Li[k * 6 + i], Li[k * 6 + j], a);
                a = spd ? a : nan;
                q[i * 6 + j] = a;
                q[j * 6 + i] = a;
            }
        // static x-y-z angles of R (tf.transformations.euler_from_matrix, axes 'sxyz'; its threshold is 4 float64 epsilons)
        const double cy = sqrt(fma(R.a[0], R.a[0], R.a[3] * R.a[3]));
        const bool reg = cy > 4.0 * 2.220446049250313e-16;
        pose[3] = reg ? atan2(R.a[7], R.a[8]) : atan2(-R.a[5], R.a[4]);
        pose[4] = atan2(-R.a[6], cy);
        pose[5] = reg ? atan2(R.a[3], R.a[0]) : 0.0;
    } else {
#pragma unroll
        for (int e = 0; e < 36; e++) c[e] = q[e] = nan;
#pragma unroll
        for (int e = 0; e < 6; e++) pose[e] = nan;
    }
    __syncthreads();          // (every lane has read its slot's words)
    if (on)
#pragma unroll
        for (int e = 0; e < 36; e++) img[lane * PM_LD + e] = c[e];
    __syncthreads();
    pm_flush<36>(img, pm_cov + g0 * 36, n, lane);
    __syncthreads();
    if (on)
#pragma unroll
        for (int e = 0; e < 36; e++) img[lane * PM_LD + e] = q[e];
    __syncthreads();
    pm_flush<36>(img, pm_info + g0 * 36, n, lane);
    __syncthreads();
    if (on)
#pragma unroll
        for (int e = 0; e < 6; e++) img[lane * PM_LD + e] = pose[e];
    __syncthreads();
    pm_flush<6>(img, pm_pose + g0 * 6, n, lane);
}
// every keyframe of every window's range: (tiles of 64 keyframes, windows); a tile beyond its window's range returns at once
void launch_pose_marginals(const View& v, const int* failed, const double* sig, double* pm_cov, double* pm_info, double* pm_pose,
                           int* pm_range, hipStream_t s) {
    hipLaunchKernelGGL(k_pose_marginals, dim3((v.M + 63) / 64, v.B), dim3(64), 0, s, v, failed, sig, pm_cov, pm_info, pm_pose, pm_range);
}
