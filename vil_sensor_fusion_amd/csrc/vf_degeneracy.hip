// vf_degeneracy.hip -- K6: batched degeneracy metrics on 6x6 information / covariance matrices,
// their 3x3 translation / rotation blocks and the 1x1 entry of each axis, one lane per message,
// everything in registers; several of those subsets of one metric in one launch (k_degeneracy_scores).
//
// Replaces the per-message numpy/LAPACK calls of the reference's metric library
// (vil_fusion/python/degeneracy_detection_functions.py:38-251) as driven by
// apply_degen_function (vil_fusion/python/make_prettier_graphs.py:547-576) and by the online
// node (vil_fusion/src/vil_fusion/degeneracy_detection.py:115-130), and the shipped float32
// D-optimality gate (gtsam_fusion/src/degerate_odometry_filter.cpp:29-47).
//
// Small-matrix kernels: Householder tridiagonalisation + implicit QL for symmetric eigenvalues, one-sided
// (Hestenes) Jacobi for singular values, LU with partial pivoting for det / inverse, all with compile-time
// indices so a 6x6 lives in 36 registers.  float64 and float32 instantiations (fp32 tolerance sweep).
//
// Layout: the small-matrix routines; the Metric enum with metric_traits (what a metric reads); the metric functions, which
// take blocks and return values (spectrum_metrics: the three of SPECTRUM); then what owns memory: stage_series_tile (HBM ->
// LDS image), pick_block (image -> registers), score_block with Put (values -> output rows), and the three kernels --
// k_degeneracy (one subset, image in two halves: more waves per SIMD), k_degeneracy_scores (any subsets of a mask from one
// image) and k_degeneracy_scores_windows (the same over an engine's windows) --, the covariance remapping of a scan's Hessian
// (jacobi_eig6: cyclic Jacobi WITH eigenvectors; k_remap_covariance, vf_degeneracy_remap_batch) and the C entry points.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "../../include/vilfusion.h"
#include "vf_kernels.hpp"
#include "vf_device_buf.hpp"

extern "C" void vf_set_last_error_(const char* msg);

namespace {

#define DI __device__ __forceinline__

template <typename T> struct Lim;
template <> struct Lim<double> { static constexpr double eps = 2.220446049250313e-16; static constexpr int sweeps = 12; };
template <> struct Lim<float> { static constexpr float eps = 1.1920929e-07f; static constexpr int sweeps = 8; };

template <typename T> DI T t_sqrt(T x) { return sqrt(x); }
template <typename T> DI T t_abs(T x) { return fabs(x); }

// Reciprocal and reciprocal square root for the Jacobi rotations: the hardware approximations (v_rcp / v_rsq: 2^-23
// relative in float64, 1 ulp in float32) + ONE third-order correction step in float64 (error e^3 ~ 2^-69: full double).
// No scaling for denormals / huge arguments as the library sqrt() and '/' carry (about 20 instructions each in float64):
// the arguments here are sums of squares of matrix entries, and the kernels document their range (|entry| in 1e-150 ... 1e150).
DI double rsq_full(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    const double e = fma(-(x * y), y, 1.0);
    return fma(y * e, fma(e, 0.375, 0.5), y);
}
DI float rsq_full(float x) { return __builtin_amdgcn_rsqf(x); }
DI double rcp_full(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, r, 1.0);
    return fma(r, fma(e, e, e), r);
}
DI float rcp_full(float x) { return __builtin_amdgcn_rcpf(x); }

// Jacobi rotation that annihilates beta in [[a, beta], [beta, b]], alpha = (b - a) / 2:
//   t = tan(phi) = sgn(alpha) beta / (|alpha| + sqrt(alpha^2 + beta^2)),  c = 1 / sqrt(1 + t^2),  s = t c
// (the textbook theta = alpha / beta form costs two divisions and two square roots; this one a reciprocal square root, a
// reciprocal and a second reciprocal square root).  beta = 0 gives t = 0, c = 1, s = 0 without a branch.
template <typename T>
DI void jacobi_cs(T alpha, T beta, T& t, T& c, T& s) {
    const T h2 = fma(alpha, alpha, beta * beta);
    const T h = h2 * rsq_full(h2 > T(0) ? h2 : T(1));
    const T den = copysign(t_abs(alpha) + h, alpha);
    t = beta != T(0) ? beta * rcp_full(den) : T(0);
    c = rsq_full(fma(t, t, T(1)));
    s = t * c;
}

// Symmetric eigenvalues by Householder tridiagonalisation + implicit QL with Wilkinson shifts and deflation, all in registers
// (compile-time indices; what varies from lane to lane -- where the unreduced block ends, whether a lane has converged -- is
// carried by selects, never by an index).  The metrics need the two ends of the spectrum only, and a full cyclic Jacobi
// (5-7 sweeps of 15 rotations, every rotation touching two rows and two columns: 4 900 vector instructions per wave for a 6 x 6)
// pays for eigenvectors nobody asked for; here the N - 2 reflections cost ~250 instructions and every QL iteration is N - 1 - l
// rotations of a tridiagonal (three numbers each): ~1 800 in all.  Accuracy is that of LAPACK's tridiagonal QL -- absolute,
// eps * |A| -- which is what the reference's own numpy.linalg.eigvals / cond deliver (Jacobi's relative accuracy on graded
// matrices is not needed: tests/test_gpu_degeneracy.py holds e_opt to 1e-9 * max|A|).  The upper triangle of `a` is read;
// a is destroyed.
template <typename T, int N>
DI void sym_eig(T (&a)[N * N], T (&d)[N], bool active) {
    T e[N];          // e[k] couples k and k + 1; e[N - 1] = 0 is the sentinel of the QL loop
#pragma unroll
    for (int k = 0; k < N; k++) e[k] = T(0);
    // ---- Householder: rows i = N-1 .. 2 of the lower triangle (held as a[c * N + r], c <= r: the upper triangle of the array)
#define SA(r, c) a[((r) < (c) ? (r) : (c)) * N + ((r) < (c) ? (c) : (r))]
#pragma unroll
    for (int i = N - 1; i >= 2; i--) {
        T tail = T(0);      // what the reflection has to annihilate: row i, columns 0 .. i-2
#pragma unroll
        for (int k = 0; k < i - 1; k++) tail = fma(SA(i, k), SA(i, k), tail);
        const T xl = SA(i, i - 1);
        const T sigma = fma(xl, xl, tail);
        const bool skip = !(tail > T(0));                 // already tridiagonal here (or a lane without a matrix)
        const T nrm = sigma * rsq_full(skip ? T(1) : sigma);
        const T alpha = -copysign(nrm, xl);
        const T h = fma(-xl, alpha, sigma);                // = v.v / 2 with v = x - alpha e
        const T inv_h = skip ? T(0) : rcp_full(h);
        T v[N], pv[N];
#pragma unroll
        for (int k = 0; k < i; k++) v[k] = skip ? T(0) : (k == i - 1 ? xl - alpha : SA(i, k));
        T f = T(0);
#pragma unroll
        for (int j = 0; j < i; j++) {
            T g = T(0);
#pragma unroll
            for (int k = 0; k < i; k++) g = fma(SA(j, k), v[k], g);
            pv[j] = g * inv_h;
            f = fma(pv[j], v[j], f);
        }
        const T hh = T(0.5) * f * inv_h;
#pragma unroll
        for (int j = 0; j < i; j++) pv[j] = fma(-hh, v[j], pv[j]);
#pragma unroll
        for (int j = 0; j < i; j++)
#pragma unroll
            for (int k = 0; k <= j; k++) SA(j, k) = SA(j, k) - fma(v[j], pv[k], pv[j] * v[k]);
        e[i - 1] = skip ? xl : alpha;
    }
    if (N >= 2) e[0] = SA(1, 0);
#pragma unroll
    for (int k = 0; k < N; k++) d[k] = SA(k, k);
#undef SA
    // ---- implicit QL (the classical tqli recurrence), eigenvalue by eigenvalue
#pragma unroll
    for (int l = 0; l < N - 1; l++) {
#pragma unroll 1
        for (int iter = 0; iter < 40; iter++) {
            int m = N - 1;                                  // the smallest m >= l whose coupling to m + 1 is negligible
#pragma unroll
            for (int k = N - 2; k >= l; k--) {
                const T dd = t_abs(d[k]) + t_abs(d[k + 1]);
                m = (t_abs(e[k]) <= Lim<T>::eps * dd) ? k : m;
            }
            const bool work = active && m != l;
            if (!__any(work)) break;
            const T el = work ? e[l] : T(1);
            T g = (d[l + 1] - d[l]) * rcp_full(el + el);
            T r2 = fma(g, g, T(1));
            T r = r2 * rsq_full(r2);
            T dm = d[N - 1];
#pragma unroll
            for (int k = N - 2; k > l; k--) dm = (m == k) ? d[k] : dm;
            g = dm - d[l] + el * rcp_full(g + copysign(r, g));
            T sn = T(1), cs = T(1), pp = T(0);
            bool brk = false;
            // (the lanes that take no part in a rotation are masked off by the branch, not by selects on every result: a
            // rotation is ~26 vector instructions this way, ~40 with selects)
#pragma unroll
            for (int i = N - 2; i >= l; i--) {
                if (work && i < m && !brk) {
                    const T f = sn * e[i], b = cs * e[i];
                    const T rr = fma(f, f, g * g);
                    if (!(rr > T(0))) {              // (underflow: the block has split here)
                        e[i + 1] = T(0);
                        d[i + 1] -= pp;
                        brk = true;
                    } else {
                        const T inv = rsq_full(rr);
                        e[i + 1] = rr * inv;
                        sn = f * inv;
                        cs = g * inv;
                        const T gg = d[i + 1] - pp;
                        const T rot = fma(d[i] - gg, sn, T(2) * cs * b);
                        pp = sn * rot;
                        d[i + 1] = gg + pp;
                        g = fma(cs, rot, -b);
                    }
                }
            }
            if (work && !brk) { d[l] -= pp; e[l] = g; }
#pragma unroll
            for (int k = l; k < N; k++) e[k] = (work && m == k) ? T(0) : e[k];
        }
    }
}

// singular values of a general matrix, one-sided (Hestenes) Jacobi on the columns; a sweep in which no lane of the wave
// rotated ends the iteration
template <typename T, int N>
DI void jacobi_svd(T (&a)[N * N], T (&sv)[N], bool active) {
#pragma unroll 1
    for (int sweep = 0; sweep < Lim<T>::sweeps; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                T al = 0, be = 0, ga = 0;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    al = fma(a[k * N + p], a[k * N + p], al);
                    be = fma(a[k * N + q], a[k * N + q], be);
                    ga = fma(a[k * N + p], a[k * N + q], ga);
                }
                constexpr T tol = Lim<T>::eps * T(0.01);
                const bool need = ga * ga > tol * tol * al * be;
                rotated |= need;
                T t, c, s;
                jacobi_cs<T>(T(0.5) * (be - al), need ? ga : T(0), t, c, s);
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const T akp = a[k * N + p], akq = a[k * N + q];
                    a[k * N + p] = fma(c, akp, -(s * akq));
                    a[k * N + q] = fma(s, akp, c * akq);
                }
            }
        if (__all(!active || !rotated)) break;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        T s = 0;
#pragma unroll
        for (int k = 0; k < N; k++) s = fma(a[k * N + i], a[k * N + i], s);
        sv[i] = t_sqrt(s);
    }
}

template <typename T> DI void swap(T& x, T& y) { const T t = x; x = y; y = t; }

// Partial pivoting at column c: the row among c .. N-1 with the largest |entry| in that column changes places with row c (by
// predicated moves), in `a` and in every matrix of `more` alike.  True if rows moved.
template <typename T, int N, typename... More>
DI bool pivot_swap(int c, T (&a)[N * N], More&... more) {
    int piv = c;
    T best = t_abs(a[c * N + c]);
    // (every row with those up to c skipped, not `r = c + 1 ..`: a trip count that depends on the argument is not unrolled in
    // a function of its own, and the matrix went to scratch, 36 words per lane)
#pragma unroll
    for (int r = 1; r < N; r++)
        if (r > c) {
            const T v = t_abs(a[r * N + c]);
            if (v > best) { best = v; piv = r; }
        }
#pragma unroll
    for (int r = 1; r < N; r++)
        if (r > c && piv == r) {
#pragma unroll
            for (int k = 0; k < N; k++) { swap(a[c * N + k], a[r * N + k]); (swap(more[c * N + k], more[r * N + k]), ...); }
        }
    return piv != c;
}

// LU with partial pivoting: each(pivot) for the pivots in elimination order, every one as soon as it is known (what `each` does
// with it overlaps the row updates that follow: a float64 log is some fifty instructions); true if the number of row swaps is odd
template <typename T, int N, typename Each>
DI bool lu_pivots(const T (&m)[N * N], Each&& each) {
    T a[N * N];
#pragma unroll
    for (int i = 0; i < N * N; i++) a[i] = m[i];
    bool odd = false;
#pragma unroll
    for (int c = 0; c < N; c++) {
        odd ^= pivot_swap<T, N>(c, a);
        const T d = a[c * N + c];
        each(d);
        const T inv = T(1) / d;
#pragma unroll
        for (int r = c + 1; r < N; r++) {
            const T f = a[r * N + c] * inv;
#pragma unroll
            for (int k = c + 1; k < N; k++) a[r * N + k] = fma(-f, a[c * N + k], a[r * N + k]);
        }
    }
    return odd;
}

// log|det| as numpy.linalg.slogdet()[1]: the logs of the pivots, summed in elimination order
template <typename T, int N>
DI T lu_logabsdet(const T (&m)[N * N]) {
    T logabs = T(0);
    lu_pivots<T, N>(m, [&](T d) __attribute__((always_inline)) { logabs += log(t_abs(d)); });
    return logabs;
}

// plain determinant: the pivots multiplied in elimination order, with the swap parity applied (a change of sign is exact, so
// it commutes with the product)
template <typename T, int N>
DI T lu_det(const T (&m)[N * N]) {
    T det = T(1);
    const bool odd = lu_pivots<T, N>(m, [&](T d) __attribute__((always_inline)) { det *= d; });
    return odd ? -det : det;
}

// inverse by Gauss-Jordan with partial pivoting
template <typename T, int N>
DI void gj_inverse(const T (&m)[N * N], T (&inv)[N * N]) {
    T a[N * N];
#pragma unroll
    for (int i = 0; i < N * N; i++) { a[i] = m[i]; inv[i] = T(0); }
#pragma unroll
    for (int i = 0; i < N; i++) inv[i * N + i] = T(1);
#pragma unroll
    for (int c = 0; c < N; c++) {
        pivot_swap<T, N>(c, a, inv);
        const T ip = T(1) / a[c * N + c];
#pragma unroll
        for (int k = 0; k < N; k++) { a[c * N + k] *= ip; inv[c * N + k] *= ip; }
#pragma unroll
        for (int r = 0; r < N; r++)
            if (r != c) {
                const T f = a[r * N + c];
#pragma unroll
                for (int k = 0; k < N; k++) {
                    a[r * N + k] = fma(-f, a[c * N + k], a[r * N + k]);
                    inv[r * N + k] = fma(-f, inv[c * N + k], inv[r * N + k]);
                }
            }
    }
}

template <typename T, int N>
DI void matmul(const T (&a)[N * N], const T (&b)[N * N], T (&c)[N * N]) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) {
            T s = 0;
#pragma unroll
            for (int k = 0; k < N; k++) s = fma(a[i * N + k], b[k * N + j], s);
            c[i * N + j] = s;
        }
}

// eigenvalues of now * prev^-1 for SPD prev: similar to L^-1 now L^-T with prev = L L^T
template <typename T, int N>
DI void ratio_eig(const T (&now)[N * N], const T (&prev)[N * N], T (&ev)[N], bool& ok, bool active) {
    T L[N * N];
#pragma unroll
    for (int i = 0; i < N * N; i++) L[i] = T(0);
    ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        T s = prev[j * N + j];
#pragma unroll
        for (int k = 0; k < j; k++) s = fma(-L[j * N + k], L[j * N + k], s);
        if (!(s > T(0))) { ok = false; s = T(1); }
        const T ljj = t_sqrt(s);
        L[j * N + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            T v = T(0.5) * (prev[i * N + j] + prev[j * N + i]);
#pragma unroll
            for (int k = 0; k < j; k++) v = fma(-L[i * N + k], L[j * N + k], v);
            L[i * N + j] = v / ljj;
        }
    }
    // Y = L^-1 now (forward substitution on each column), S = Y L^-T (same on rows)
    T Y[N * N], S[N * N];
#pragma unroll
    for (int c = 0; c < N; c++)
#pragma unroll
        for (int r = 0; r < N; r++) {
            T v = T(0.5) * (now[r * N + c] + now[c * N + r]);
#pragma unroll
            for (int k = 0; k < r; k++) v = fma(-L[r * N + k], Y[k * N + c], v);
            Y[r * N + c] = v / L[r * N + r];
        }
#pragma unroll
    for (int r = 0; r < N; r++)
#pragma unroll
        for (int c = 0; c < N; c++) {
            T v = Y[r * N + c];
#pragma unroll
            for (int k = 0; k < c; k++) v = fma(-L[c * N + k], S[r * N + k], v);
            S[r * N + c] = v / L[c * N + c];
        }
#pragma unroll
    for (int r = 0; r < N; r++)
#pragma unroll
        for (int c = r + 1; c < N; c++) { const T m = T(0.5) * (S[r * N + c] + S[c * N + r]); S[r * N + c] = m; S[c * N + r] = m; }
    sym_eig<T, N>(S, ev, active);
}

enum Metric { D_OPT, D_OPT_RATIO, A_OPT, A_OPT_RATIO, E_OPT, E_OPT_RATIO, MAX_EIGEN, MAX_EIGEN_RATIO, JENSEN_BREGMAN,
              CORR_DIST, KULLBACK_LEIBLER, NORM_FRO, NORM_FRO_RATIO, NORM_NUC, NORM_NUC_RATIO, NORM_1, NORM_1_RATIO,
              NORM_2, NORM_2_RATIO, COND_NUMBER, DIFF_ENTROPY,
              // the variants of degeneracy_detection_functions.py:184-193, 247-251
              JENSEN_BREGMAN_0, KL_0POSE, KL_0COV, CONDITION_COV, N_METRICS,
              SPECTRUM = N_METRICS };     // (not a metric of the reference: e_opt, max_eigen and condition_number of one eigen-solve, vf_degeneracy_spectrum_batch)

// What a metric reads besides the matrix of its own message (make_prettier_graphs.py:565-574): prev = the previous message's
// matrix (the ratio / divergence family), ratio = it enters as now . prev^-1, pose = the poses of both messages
struct MetricTraits { bool prev, ratio, pose; };
__host__ __device__ constexpr MetricTraits metric_traits(int m) {
    switch (m) {
        case D_OPT_RATIO: case A_OPT_RATIO: case NORM_FRO_RATIO: case NORM_NUC_RATIO: case NORM_1_RATIO: case NORM_2_RATIO:
            return {true, true, false};
        case E_OPT_RATIO: case MAX_EIGEN_RATIO: case JENSEN_BREGMAN: case CORR_DIST: case KL_0POSE:
            return {true, false, false};
        case KULLBACK_LEIBLER:
            return {true, false, true};
        default:
            return {false, false, false};
    }
}

// subset id -> (N, offset of the block on the diagonal): 0 all (6, 0), 1 trans (3, 0), 2 rot (3, 3), 3 + a the 1x1 entry of
// axis a = x y z roll pitch yaw (1, a)
constexpr int N_SUBSETS = 9;
__host__ __device__ constexpr int subset_off(int s) { return s == 2 ? 3 : (s < 3 ? 0 : s - 3); }

// numpy.linalg.cond of a 1x1: s / s = 1, and 0 / 0 -> inf (numpy turns the NaN of a singular matrix into inf)
template <typename T>
DI T cond_1x1(T a) { return a != a ? a : (t_abs(a) > T(0) ? T(1) : T(INFINITY)); }

// numpy.linalg.det of a 1x1: numpy takes every determinant as sign * exp(log|det|) of its LU factors (slogdet), so det([[x]])
// is x to within an ulp or two -- and the kullback_leibler of two close entries cancels down to exactly those ulps
template <typename T>
DI T det_1x1(T x) { return x == T(0) ? T(0) : copysign(exp(log(t_abs(x))), x); }

// The reference's numpy calls on a 1x1 [[a]] (prev [[b]], pose difference du = prev - now), in closed form.  inv() of a zero
// raises LinAlgError there: NaN here, also for the norm_*_ratio functions, which do not catch it (the reference raises).
template <typename T, int METRIC>
DI T metric_1x1(T a, T b, T du) {
    const T nan = T(NAN);
    const T r = a * (T(1) / b);          // now @ inv(prev)
    switch (METRIC) {
        case D_OPT: return exp(log(t_abs(a)));
        case D_OPT_RATIO: return b != T(0) ? exp(log(t_abs(r))) : nan;
        case A_OPT: case E_OPT: case MAX_EIGEN: return a;
        case A_OPT_RATIO: case E_OPT_RATIO: case MAX_EIGEN_RATIO: return b != T(0) ? r : nan;
        case JENSEN_BREGMAN: return log(t_abs((a + b) / T(2))) - T(0.5) * det_1x1(a * b);
        case JENSEN_BREGMAN_0: return log(t_abs(a / T(2)));
        case CORR_DIST: return (a > T(0) && b > T(0)) ? T(0) : nan;    // both "correlations" are [[1]]
        case KULLBACK_LEIBLER: case KL_0POSE: {
            if (!(a != T(0) && b != T(0))) return nan;
            const T ai = T(1) / a;
            const T d = METRIC == KL_0POSE ? T(0) : du;
            return T(0.5) * ((ai * b - T(1)) + d * (ai * d) + log(t_abs(det_1x1(a)) / t_abs(det_1x1(b))));
        }
        case KL_0COV: return nan;
        case NORM_FRO: return t_sqrt(a * a);
        case NORM_NUC: case NORM_1: case NORM_2: return t_abs(a);
        case NORM_FRO_RATIO: return b != T(0) ? t_sqrt(r * r) : nan;
        case NORM_NUC_RATIO: case NORM_1_RATIO: case NORM_2_RATIO: return b != T(0) ? t_abs(r) : nan;
        case COND_NUMBER: return -cond_1x1(a);
        case CONDITION_COV: return cond_1x1(a);
        case DIFF_ENTROPY: {
            const T d = T(2.0 * 3.141592653589793 * 2.718281828459045) * det_1x1(a);
            return d > T(0) ? T(0.5) * log(d) : nan;
        }
        default: return nan;
    }
}

template <typename T, int N>
DI T norm1(const T (&a)[N * N]) {
    T best = 0;
#pragma unroll
    for (int c = 0; c < N; c++) {
        T s = 0;
#pragma unroll
        for (int r = 0; r < N; r++) s += t_abs(a[r * N + c]);
        best = s > best ? s : best;
    }
    return best;
}
template <typename T, int N>
DI T normfro(const T (&a)[N * N]) {
    T s = 0;
#pragma unroll
    for (int i = 0; i < N * N; i++) s = fma(a[i], a[i], s);
    return t_sqrt(s);
}

constexpr int MSTRIDE = 37;   // LDS stride of one 6x6 (36 + 1 pad: 64 lanes reading entry e of their own matrix hit 32 / 64 distinct banks)

// The symmetric part (m + m^T) / 2 with the largest |m_rc - m_cr| and the largest |entry| of m
template <typename T, int N>
DI void sym_part(const T (&m)[N * N], T (&s)[N * N], T& asym, T& big) {
    asym = T(0);
    big = T(0);
#pragma unroll
    for (int r = 0; r < N; r++)
#pragma unroll
        for (int c = 0; c < N; c++) {
            s[r * N + c] = T(0.5) * (m[r * N + c] + m[c * N + r]);
            big = t_abs(m[r * N + c]) > big ? t_abs(m[r * N + c]) : big;
            if (c > r) { const T dsy = t_abs(m[r * N + c] - m[c * N + r]); asym = dsy > asym ? dsy : asym; }
        }
}
// "Symmetric" = to within rounding of the entries (an asymmetry of that size moves a singular value by as much: what the SVD's
// own rounding does)
template <typename T>
DI bool symmetric_to_rounding(T asym, T big) { return asym <= T(8) * Lim<T>::eps * big; }

// What the metrics read off a spectrum (eigenvalues, or singular values, which are their own moduli): its two ends, the two
// ends of its moduli and their sum
template <typename T>
struct Spectrum {
    T lo, hi, alo, ahi, sum;
    DI T cond() const { return ahi / alo; }       // numpy.linalg.cond of a symmetric matrix
};
template <typename T, int N>
DI Spectrum<T> spectrum_of(const T (&ev)[N]) {
    Spectrum<T> s{ev[0], ev[0], t_abs(ev[0]), t_abs(ev[0]), T(0)};
#pragma unroll
    for (int k = 0; k < N; k++) {
        const T x = t_abs(ev[k]);
        s.lo = ev[k] < s.lo ? ev[k] : s.lo; s.hi = ev[k] > s.hi ? ev[k] : s.hi;
        s.alo = x < s.alo ? x : s.alo; s.ahi = x > s.ahi ? x : s.ahi;
        s.sum += x;
    }
    return s;
}

// e_opt, max_eigen and condition_number from ONE eigen-solve of the symmetric part: e_opt and max_eigen are defined on it;
// condition_number too whenever the matrix is symmetric to rounding -- other matrices get NaN there (the SVD's business:
// COND_NUMBER below).  The single metrics E_OPT and MAX_EIGEN are members of this.
template <typename T> struct SpectrumMetrics { T e_opt, max_eigen, condition_number; };
template <typename T, int N>
DI SpectrumMetrics<T> spectrum_metrics(const T (&now)[N * N], bool active) {
    if constexpr (N == 1) {
        return {now[0], now[0], -cond_1x1(now[0])};
    } else {
        T s[N * N], ev[N], asym, big;
        sym_part<T, N>(now, s, asym, big);
        sym_eig<T, N>(s, ev, active);
        const Spectrum<T> sp = spectrum_of<T, N>(ev);
        return {sp.lo, sp.hi, symmetric_to_rounding(asym, big) ? -sp.cond() : T(NAN)};
    }
}

// One metric of a message on its N x N block, N = 6 or 3 (`now`, `prev`: the block of the message and of the one before it, the
// identity on lanes that are not `active`; du: the pose difference on the block's axes, KULLBACK_LEIBLER only).
// The wave-uniform decisions in here (__any in the QL loop of sym_eig, __all in the sweep of jacobi_svd and in front of the
// symmetric fast path) are taken over the wave's 64 consecutive messages of a series, whichever kernel calls; lanes that are
// not active hold the identity and vote for the cheap side.  Built with -ffp-contract=fast: an expression keeps its grouping.
template <typename T, int N, int METRIC>
DI T block_metric(const T (&now)[N * N], const T (&prev)[N * N], const T (&du)[N], bool active) {
    const T nan = T(NAN);
    T y = nan;
    T ratio[N * N];
    if (metric_traits(METRIC).ratio) {
        T pinv[N * N];
        gj_inverse<T, N>(prev, pinv);
        matmul<T, N>(now, pinv, ratio);
    }
    switch (METRIC) {
        case D_OPT: case D_OPT_RATIO: {
            const T la = (METRIC == D_OPT) ? lu_logabsdet<T, N>(now) : lu_logabsdet<T, N>(ratio);
            y = exp(la / T(N));
        } break;
        case A_OPT: case A_OPT_RATIO: {
            T s = 0;
#pragma unroll
            for (int k = 0; k < N; k++) s += (METRIC == A_OPT) ? now[k * N + k] : ratio[k * N + k];
            y = s;
        } break;
        case E_OPT: y = spectrum_metrics<T, N>(now, active).e_opt; break;
        case MAX_EIGEN: y = spectrum_metrics<T, N>(now, active).max_eigen; break;
        case E_OPT_RATIO: case MAX_EIGEN_RATIO: {
            T ev[N];
            bool ok;
            ratio_eig<T, N>(now, prev, ev, ok, active);
            const Spectrum<T> sp = spectrum_of<T, N>(ev);
            y = ok ? (METRIC == E_OPT_RATIO ? sp.lo : sp.hi) : nan;
        } break;
        case JENSEN_BREGMAN: {
            T avg[N * N], prod[N * N];
#pragma unroll
            for (int k = 0; k < N * N; k++) avg[k] = (now[k] + prev[k]) / T(2);
            matmul<T, N>(now, prev, prod);
            y = lu_logabsdet<T, N>(avg) - T(0.5) * lu_det<T, N>(prod);
        } break;
        case JENSEN_BREGMAN_0: {   // jensen_bregman(now, 0): slogdet(now / 2)[1] - 0.5 det(now @ 0), and numpy's det of the zero
                                   // matrix is 0 (lu_det's would be 0 * (1 / 0) = NaN: not the JENSEN_BREGMAN path with prev = 0)
            T half[N * N];
#pragma unroll
            for (int k = 0; k < N * N; k++) half[k] = now[k] / T(2);
            y = lu_logabsdet<T, N>(half);
        } break;
        case KL_0COV: break;       // kullback_leibler(now, 0, ...) inverts the zero matrix: LinAlgError, NaN for every message
        case CORR_DIST: {   // elementwise-product quirk: only the diagonal of the "correlation" survives
            T tr = 0, fx = 0, fy = 0;
            bool ok = true;
#pragma unroll
            for (int k = 0; k < N; k++) {
                const T dn = t_sqrt(now[k * N + k]), dp = t_sqrt(prev[k * N + k]);
                if (!(dn > T(0)) || !(dp > T(0))) ok = false;
                const T cn = (T(1) / dn) * now[k * N + k] * (T(1) / dn), cp = (T(1) / dp) * prev[k * N + k] * (T(1) / dp);
                tr = fma(cn, cp, tr);
                fx = fma(cn, cn, fx);
                fy = fma(cp, cp, fy);
            }
            y = ok ? T(1) - tr / (t_sqrt(fx) * t_sqrt(fy)) : nan;
        } break;
        case KULLBACK_LEIBLER: case KL_0POSE: {   // E1 = prev, E2 = now; KL_0POSE: pose difference 0 (du is)
            // (the determinants first: `now` is not needed past the inversion then, and du is carried through it)
            const T c = log(t_abs(lu_det<T, N>(now)) / t_abs(lu_det<T, N>(prev)));
            T e2i[N * N], m[N * N];
            gj_inverse<T, N>(now, e2i);
            matmul<T, N>(e2i, prev, m);
            T a = 0, b = 0;
#pragma unroll
            for (int k = 0; k < N; k++) a += m[k * N + k] - T(1);
#pragma unroll
            for (int r = 0; r < N; r++) {
                T s = 0;
#pragma unroll
                for (int c = 0; c < N; c++) s = fma(e2i[r * N + c], du[c], s);
                b = fma(du[r], s, b);
            }
            y = T(0.5) * (a + b + c);
        } break;
        case NORM_FRO: y = normfro<T, N>(now); break;
        case NORM_FRO_RATIO: y = normfro<T, N>(ratio); break;
        case NORM_1: y = norm1<T, N>(now); break;
        case NORM_1_RATIO: y = norm1<T, N>(ratio); break;
        case NORM_NUC: case NORM_2: case COND_NUMBER: case CONDITION_COV: case NORM_NUC_RATIO: case NORM_2_RATIO: {
            T w[N * N], sv[N];
            constexpr bool r = metric_traits(METRIC).ratio;
            // the nuclear norm, the 2-norm or the condition number of a spectrum; CONDITION_COV = +cond, the same bits negated
            auto of = [](const Spectrum<T>& sp) {
                if (METRIC == NORM_NUC || METRIC == NORM_NUC_RATIO) return sp.sum;
                if (METRIC == COND_NUMBER) return -sp.cond();
                return METRIC == CONDITION_COV ? sp.cond() : sp.ahi;
            };
            if (!r) {
                // An information matrix is symmetric, and the singular values of a symmetric matrix are the moduli of its
                // eigenvalues: sigma_max / sigma_min, the sum and the maximum come from the eigen-solve e_opt / max_eigen use, at a
                // seventh of the cost of a Jacobi SVD.  A wave with a lane that holds anything else takes the general path below.
                T asym, big;
                sym_part<T, N>(now, w, asym, big);
                if (__all(!active || symmetric_to_rounding(asym, big))) {
                    sym_eig<T, N>(w, sv, active);
                    y = of(spectrum_of<T, N>(sv));
                    break;
                }
            }
#pragma unroll
            for (int k = 0; k < N * N; k++) w[k] = r ? ratio[k] : now[k];
            jacobi_svd<T, N>(w, sv, active);
            y = of(spectrum_of<T, N>(sv));
        } break;
        case DIFF_ENTROPY: {
            const T x = pow(T(2.0 * 3.141592653589793 * 2.718281828459045), T(N));
            const T d = x * lu_det<T, N>(now);
            y = d > T(0) ? T(0.5) * log(d) : nan;
        } break;
        default: break;
    }
    return y;
}

// One metric on the N x N block of any subset: N = 1 (the per-axis subsets) takes the closed forms of metric_1x1
template <typename T, int N, int METRIC>
DI T degeneracy_metric(const T (&now)[N * N], const T (&prev)[N * N], const T (&du)[N], bool active) {
    if constexpr (N == 1) return metric_1x1<T, METRIC>(now[0], prev[0], du[0]);
    else return block_metric<T, N, METRIC>(now, prev, du, active);
}

// Where a lane's values go: entry i of one output row after another, `row` values apart.  The first message of a series has
// nothing in front of it and scores 0 (make_prettier_graphs.py:562-563); lanes past the end of the series store nothing.
template <typename T>
struct Put {
    T* __restrict__ o;
    size_t row;
    int i, count;
    DI void operator()(T y) {
        if (i == 0) o[0] = T(0);
        else if (i < count) o[i] = y;
        o += row;
    }
};

// Message i's values of METRIC on the N x N block at `off`: one, or the three of SPECTRUM
template <typename T, int N, int METRIC>
DI Put<T> score_block(const T (&now)[N * N], const T (&prev)[N * N], const T* __restrict__ pose, int i, int off, bool active, Put<T> put) {
    if constexpr (METRIC == SPECTRUM) {
        const SpectrumMetrics<T> s = spectrum_metrics<T, N>(now, active);
        put(s.e_opt);
        put(s.max_eigen);
        put(s.condition_number);
    } else {
        T du[N];     // the pose of the message before, minus this one's
#pragma unroll
        for (int k = 0; k < N; k++)
            du[k] = (metric_traits(METRIC).pose && pose && active) ? pose[(size_t)(i - 1) * 6 + off + k] - pose[(size_t)i * 6 + off + k] : T(0);
        put(degeneracy_metric<T, N, METRIC>(now, prev, du, active));
    }
    return put;
}

// the N x N block at (off, off) of the 6 x 6 staged at `m` (LDS), or the identity on a lane that is not active
template <typename T, int N>
DI void pick_block(const T* m, int off, bool active, T (&a)[N * N]) {
#pragma unroll
    for (int r = 0; r < N; r++)
#pragma unroll
        for (int c = 0; c < N; c++) a[r * N + c] = active ? m[off * 7 + r * 6 + c] : T(r == c);
}

// Staging: the TILE matrices of the series from `base` on (those that exist: the series has `count`), and with PREV the one in
// front of them, are ONE contiguous stretch of HBM; it is copied into the LDS image (matrix base + l at local index l + 1, the
// one in front at 0) with 16-byte loads, fully coalesced, FLIGHT of them per lane (0: all) issued before the first is waited for
// (they are 4 registers of the lane each while they fly).  Every lane then picks its own matrix out of LDS (lane = message reads
// of 288-byte records straight from HBM touch 64 cache lines per load instruction).
template <typename T, bool PREV, int TILE, int FLIGHT>
DI void stage_series_tile(T* __restrict__ lds, const T* __restrict__ mats, int base, int count, int lane) {
    const int first = (PREV && base > 0) ? base - 1 : base;           // first matrix staged, local index first - base + 1
    const int last = base + TILE < count ? base + TILE : count;
    constexpr int V = 16 / (int)sizeof(T);                             // elements per 16-byte load (36 is a multiple of both)
    constexpr int PER = ((TILE + 1) * 36 / V + 63) / 64;               // 16-byte loads per lane at most
    const int nvec = (last - first) * 36 / V;
    using vec_t = T __attribute__((ext_vector_type(V)));
    const vec_t* src = reinterpret_cast<const vec_t*>(mats + (size_t)first * 36);
    constexpr int F = FLIGHT ? FLIGHT : PER;
    // (the groups in a rolled loop that a lane leaves when it has run out of vectors: unrolled, the LDS addresses of every group
    // are computed up front and a kernel that stages at four or more waves per SIMD loses one of them to the registers; a fixed
    // number of rounds with every load and store predicated cost k_degeneracy 3-5 % at 2^22 matrices,
    // profiles/k6_one_path_timing.json)
#pragma unroll 1
    for (int v0 = lane; v0 < nvec; v0 += 64 * F) {
        vec_t x[F];
#pragma unroll
        for (int k = 0; k < F; k++)
            if (k == 0 || v0 + 64 * k < nvec) x[k] = __builtin_nontemporal_load(src + v0 + 64 * k);
#pragma unroll
        for (int k = 0; k < F; k++) {
            const int v = v0 + 64 * k;
            if (k == 0 || v < nvec) {
                const int e = v * V, m = e / 36, r = e - m * 36;
                T* dst = lds + (m + first - base + 1) * MSTRIDE + r;
#pragma unroll
                for (int j = 0; j < V; j++) dst[j] = x[k][j];
            }
        }
        if (F == PER) break;         // one group holds them all: no loop
    }
}

// mats: (T,6,6) row-major, pose (T,6) or null; N and off from the subset (6 / 3 / 1, subset_off); out: one row of `count`
// values (SPECTRUM: three).  One wave per 64 consecutive messages.  METRIC is a template parameter: a metric's kernel
// contains only its own arithmetic and loads the previous matrix only if it uses it.
template <typename T, int N, int METRIC>
__global__ void __launch_bounds__(64) k_degeneracy(const T* __restrict__ mats, const T* __restrict__ pose, int count, int off,
                                                   T* __restrict__ out) {
    // staged in two halves of 32 messages (lanes 0-31 pick theirs up after the first, 32-63 after the second): 9.8 KB of LDS
    // per wave instead of 19.2, i.e. four waves per SIMD instead of two for the Jacobi kernels; with that many waves to hide a
    // load behind, one load in flight per lane (the matrices of the first half are in registers while the second is staged)
    __shared__ T lds[33 * MSTRIDE];
    const int lane = threadIdx.x, base = blockIdx.x * 64;
    const int i = base + lane;
    constexpr bool PREV = metric_traits(METRIC).prev;
    const bool active = i > 0 && i < count;
    T now[N * N], prev[N * N];
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int hb = base + 32 * half;                                  // first message of this half
        if (half) __syncthreads();
        if (hb < count) stage_series_tile<T, PREV, 32, 1>(lds, mats, hb, count, lane);
        __syncthreads();
        if ((lane >> 5) == half) {
            const int l = lane & 31;
            pick_block<T, N>(lds + (l + 1) * MSTRIDE, off, active, now);
            pick_block<T, N>(lds + l * MSTRIDE, off, PREV && active, prev);
        }
    }
    score_block<T, N, METRIC>(now, prev, pose, i, off, active, Put<T>{out, (size_t)count, i, count});
}

// What the two fused kernels below do with the image of a tile of 64: every subset set in `mask` for message i = base + lane
// of the series, one after another (subsets in sequence, not interleaved: the registers are those of the largest one).  out:
// one row per subset in the mask, in ascending subset id, `row` values apart; the lane's value goes to entry i of each.
template <typename T, int METRIC>
DI void scores_from_image(const T* __restrict__ lds, const T* __restrict__ pose, int i, int count, unsigned mask, T* __restrict__ out,
                          size_t row, int lane) {
    constexpr bool PREV = metric_traits(METRIC).prev;
    const bool active = i > 0 && i < count;
    const T* mn = lds + (lane + 1) * MSTRIDE;
    const T* mp = lds + lane * MSTRIDE;
    Put<T> put{out, row, i, count};
    auto subset = [&](auto N, int s) __attribute__((always_inline)) {
        T now[N() * N()], prev[N() * N()];
        pick_block<T, N()>(mn, subset_off(s), active, now);
        pick_block<T, N()>(mp, subset_off(s), PREV && active, prev);
        put = score_block<T, N(), METRIC>(now, prev, pose, i, subset_off(s), active, put);
    };
    if (mask & 1u) subset(std::integral_constant<int, 6>{}, 0);
#pragma unroll 1
    for (int s = 1; s < 3; s++)
        if (mask >> s & 1u) subset(std::integral_constant<int, 3>{}, s);
#pragma unroll 1
    for (int s = 3; s < N_SUBSETS; s++)
        if (mask >> s & 1u) subset(std::integral_constant<int, 1>{}, s);
}

// Several subsets of one metric in one launch (the online node's score_all / score_trans / score_rot of one message,
// vil_fusion/src/vil_fusion/degeneracy_detection.py:115-130): the wave's 64 matrices (and the one before them) are staged
// into LDS ONCE and every subset set in `mask` is then evaluated from that image, one after another, by the arithmetic of
// k_degeneracy over the same 64 messages: a row has the bits of the launch of its subset alone.  out: one row of `count`
// values per subset in the mask, in ascending subset id.  All 65 matrices stay in LDS for the whole launch (19.2 KB per wave
// in float64).
template <typename T, int METRIC>
__global__ void __launch_bounds__(64) k_degeneracy_scores(const T* __restrict__ mats, const T* __restrict__ pose, int count,
                                                          unsigned mask, T* __restrict__ out) {
    __shared__ T lds[65 * MSTRIDE];
    const int lane = threadIdx.x, base = blockIdx.x * 64;
    stage_series_tile<T, metric_traits(METRIC).prev, 64, 0>(lds, mats, base, count, lane);
    __syncthreads();
    scores_from_image<T, METRIC>(lds, pose, base + lane, count, mask, out, (size_t)count, lane);
}

// The same over the windows of an engine, from records that are on the device already (the pose marginals vf_engine_marginals_ex
// leaves with VF_MARGINALS_POSE: kernels/kpose.inc): grid (tiles of 64 keyframes, windows).  mats / pose hold one record per
// keyframe slot, [windows x M]; the range [lo, hi) of window w (range[2 w], range[2 w + 1]) is a series of its own -- the
// score of keyframe lo is 0, and `prev` never reaches into another window or in front of lo.  Tile t of a window is messages
// 64 t .. 64 t + 63 of that series, so the wave-uniform decisions inside the metrics are taken over the same 64 messages as in
// k_degeneracy_scores run on the window's records alone, and the bits are the same.  out: one row of windows x M values per
// subset in the mask; the value of a keyframe sits at its slot.  float64 only (the records are).
template <int METRIC>
__global__ void __launch_bounds__(64) k_degeneracy_scores_windows(const double* __restrict__ mats, const double* __restrict__ pose,
                                                                  const int* __restrict__ range, int M, size_t row, unsigned mask,
                                                                  double* __restrict__ out) {
    __shared__ double lds[65 * MSTRIDE];
    const int w = blockIdx.y, lane = threadIdx.x, base = blockIdx.x * 64;
    const int lo = range[2 * w], count = range[2 * w + 1] - lo;
    if (base >= count || lo < 0 || lo + count > M) return;
    const size_t g0 = (size_t)w * M + lo;
    stage_series_tile<double, metric_traits(METRIC).prev, 64, 0>(lds, mats + g0 * 36, base, count, lane);
    __syncthreads();
    scores_from_image<double, METRIC>(lds, pose + g0 * 6, base + lane, count, mask, out + g0, row, lane);
}

// metric id -> its instantiation: f(std::integral_constant<int, M>{}) for M = metric; an id out of range calls nothing
template <int M = 0, typename F>
void with_metric(int metric, F&& f) {
    if constexpr (M < N_METRICS) {
        if (metric == M) f(std::integral_constant<int, M>{});
        else with_metric<M + 1>(metric, f);
    }
}
static_assert(N_METRICS == 25, "the metric ids of include/vilfusion.h (with_metric reaches every one of them)");
static_assert(N_METRICS == vf::K6_METRICS && N_SUBSETS == vf::K6_SUBSETS, "what vf_engine_marginal_scores checks its arguments against");

// degerate_odometry_filter.cpp:29-47 (float32): hessian (row-major floats) copied into a
// column-major Eigen matrix, rotation = block(3,3), translation = block(0,0), log(det)
__global__ void k_dopt_filter(const float* __restrict__ h, int count, float rot_thr, float trans_thr,
                              float* __restrict__ rot, float* __restrict__ trans, unsigned char* __restrict__ keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float* m = h + (size_t)i * 36;
    auto det3 = [&](int o) {   // Eigen(r,c) = m[c*6 + r]
        auto E = [&](int r, int c) { return m[(o + c) * 6 + o + r]; };
        return E(0, 0) * (E(1, 1) * E(2, 2) - E(1, 2) * E(2, 1)) - E(0, 1) * (E(1, 0) * E(2, 2) - E(1, 2) * E(2, 0)) +
               E(0, 2) * (E(1, 0) * E(2, 1) - E(1, 1) * E(2, 0));
    };
    const float r = logf(det3(3)), t = logf(det3(0));
    rot[i] = r;
    trans[i] = t;
    keep[i] = !(r < rot_thr || t < trans_thr);
}

// ---- covariance remapping (vf_degeneracy_remap_batch): the directions a scan did not observe are deweighted, not dropped.
//   Hs = (H + H^T) / 2,  H' = D Hs D with D = diag(trans_thr^-1/2 x 3, rot_thr^-1/2 x 3),  H' = V diag(l') V^T,
//   g_i = clamp(l'_i, floor, 1),  Sigma = N + N^1/2 [sum_i (1 / g_i - 1) v_i v_i^T] N^1/2,
//   M = Sigma^-1 = N^-1/2 G N^-1/2 with G = I + sum_i (g_i - 1) v_i v_i^T,  R = chol_upper(M) = chol_upper(G) N^-1/2.
// Both sums are ADDITIVE corrections of the nominal: with every g_i = 1 their weights are exact zeros, Sigma is N and R is
// diag(nom^-1/2) to the bit.  Every product under the sums is written so that it does not depend on which of (r, c) comes
// first (w * (a * b), F * (s_r * s_c)): the block permutation of out_order = 1 permutes bits.
struct RemapParams {
    double d[6];        // D, input order [trans 3, rot 3]
    double nom[6];      // N, input order
    double s[6];        // N^1/2
    double is[6];       // N^-1/2 = 1 / sqrt(nom)
    double floor;
    int out_order;      // 1: outputs in [rot, trans]
};

// Cyclic two-sided Jacobi on the symmetric 6 x 6 held as its upper triangle u[21] (entry (r, c), r <= c, at UT(r, c)), with the
// rotations accumulated into v (columns = eigenvectors, v = I on entry); the eigenvalues are left on the diagonal.  A lane
// rotates a pair only where that pair still needs it, under its own branch: what a lane computes does not depend on the lanes
// beside it, and the sweeps a converged lane sits through leave its registers alone.  The sweep loop ends for the whole wave
// (as jacobi_svd's) once no active lane has rotated.
#define UT(r, c) ((r) * 6 - (r) * ((r) + 1) / 2 + (c))
DI void jacobi_eig6(double (&u)[21], double (&v)[36], bool active) {
    double nrm2 = 0.0;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) nrm2 = fma(u[UT(r, c)], (r == c ? 1.0 : 2.0) * u[UT(r, c)], nrm2);
    constexpr double tol2 = Lim<double>::eps * Lim<double>::eps;
    // below this an off-diagonal entry is rounding of the matrix itself (pairs whose diagonal product is zero or negative --
    // eigenvalues at or below zero -- have no relative scale of their own)
    const double tiny = tol2 * nrm2;
#pragma unroll 1
    for (int sweep = 0; sweep < Lim<double>::sweeps; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 5; p++)
#pragma unroll
            for (int q = p + 1; q < 6; q++) {
                const double app = u[UT(p, p)], aqq = u[UT(q, q)], apq = u[UT(p, q)];
                const double scale = t_abs(app * aqq);
                const bool need = apq * apq > tol2 * (scale > tiny ? scale : tiny);
                if (need) {
                    rotated = true;
                    double t, c, s;
                    jacobi_cs<double>(0.5 * (aqq - app), apq, t, c, s);
                    u[UT(p, p)] = fma(-t, apq, app);
                    u[UT(q, q)] = fma(t, apq, aqq);
                    u[UT(p, q)] = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        if (k != p && k != q) {
                            double& akp = u[k < p ? UT(k, p) : UT(p, k)];
                            double& akq = u[k < q ? UT(k, q) : UT(q, k)];
                            const double x = akp, y = akq;
                            akp = fma(c, x, -(s * y));
                            akq = fma(s, x, c * y);
                        }
                        const double x = v[k * 6 + p], y = v[k * 6 + q];
                        v[k * 6 + p] = fma(c, x, -(s * y));
                        v[k * 6 + q] = fma(s, x, c * y);
                    }
                }
            }
        if (__all(!active || !rotated)) break;
    }
}

// ascending order of six values by a fixed network of 12 compare-exchanges (Bose-Nelson)
DI void sort6(double (&x)[6]) {
#define CX(i, j) { const double lo = x[i] < x[j] ? x[i] : x[j], hi = x[i] < x[j] ? x[j] : x[i]; x[i] = lo; x[j] = hi; }
    CX(1, 2) CX(4, 5) CX(0, 2) CX(3, 5) CX(0, 1) CX(3, 4) CX(2, 5) CX(0, 3) CX(1, 4) CX(2, 4) CX(1, 3) CX(2, 3)
#undef CX
}

// The wave's rows of W doubles, one per lane, from the LDS image (row of lane l at l * (W | 1): an odd stride, every bank) to
// dst, the first of them, as 16-byte vectors: n rows, consecutive lanes to consecutive vectors.  dst is 16-byte aligned (a tile
// begins at a multiple of 64 rows).
template <int W>
DI void flush_rows(const double* __restrict__ lds, double* __restrict__ dst, int n, int lane) {
    constexpr int SW = W | 1;
    using vec_t = double __attribute__((ext_vector_type(2)));
    const int total = n * W;
#pragma unroll 1
    for (int e = 2 * lane; e + 1 < total; e += 128) {
        const int m0 = e / W, m1 = (e + 1) / W;
        vec_t x;
        x[0] = lds[m0 * SW + (e - m0 * W)];
        x[1] = lds[m1 * SW + (e + 1 - m1 * W)];
        *reinterpret_cast<vec_t*>(dst + e) = x;
    }
    if ((total & 1) && lane == 0) dst[total - 1] = lds[(n - 1) * SW + W - 1];
}

// hess: (count, 6, 6) of T, promoted to float64 on load (all arithmetic is float64: a float32 call has the bits of the float64
// call on the promoted values).  One lane per message, one wave per 64.  cov (count, 36), sqrt_info (count, 21: the upper
// triangle of R by rows) or null, eig (count, 6: eigenvalues of Hs, ascending) or null, deweighted (count).  Lanes past the end
// and lanes whose matrix is not finite run on the identity; the latter report -1, Sigma = N / floor, the matching R, NaN.
template <typename T>
__global__ void __launch_bounds__(64) k_remap_covariance(const T* __restrict__ hess, int count, RemapParams P, double* __restrict__ cov,
                                                         double* __restrict__ sqrt_info, double* __restrict__ eig, int* __restrict__ deweighted) {
    __shared__ double lds[65 * MSTRIDE];
    const int lane = threadIdx.x, base = blockIdx.x * 64;
    const int i = base + lane, n = count - base < 64 ? count - base : 64;
    const bool active = i < count;
    stage_series_tile<T, false, 64, 0>(reinterpret_cast<T*>(lds), hess, base, count, lane);
    __syncthreads();
    T raw[36];
    pick_block<T, 6>(reinterpret_cast<const T*>(lds) + (lane + 1) * MSTRIDE, 0, active, raw);
    __syncthreads();          // every lane has its matrix: the image is free for the outputs
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 36; k++) finite = finite && t_abs((double)raw[k]) < (double)INFINITY;
    const bool solve = active && finite;
    double hs[36], u[21], v[36];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 6; c++) {
            hs[r * 6 + c] = solve ? 0.5 * ((double)raw[r * 6 + c] + (double)raw[c * 6 + r]) : double(r == c);
            v[r * 6 + c] = double(r == c);
        }
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) u[UT(r, c)] = solve ? hs[r * 6 + c] * (P.d[r] * P.d[c]) : double(r == c);
    const bool want_eig = eig != nullptr;
    double ev[6];
    if (want_eig) {           // (uniform) eigenvalues of Hs itself: values only, the solve the metrics use
        sym_eig<double, 6>(hs, ev, solve);
        sort6(ev);
    }
    jacobi_eig6(u, v, solve);
    // the weights of the two additive sums: exact zeros where g = 1
    double wc[6], wm[6];
    int dw = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double l = u[UT(k, k)];
        const double g = l < P.floor ? P.floor : (l > 1.0 ? 1.0 : l);
        dw += g < 1.0;
        wc[k] = 1.0 / g - 1.0;
        wm[k] = g - 1.0;
    }
    double fc[21], fm[21];       // upper triangles of sum w v v^T
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const double vv = v[r * 6 + k] * v[c * 6 + k];
                a = fma(wc[k], vv, a);
                b = fma(wm[k], vv, b);
            }
            fc[UT(r, c)] = (r == c ? P.nom[r] : 0.0) + a * (P.s[r] * P.s[c]);
            fm[UT(r, c)] = (r == c ? 1.0 : 0.0) + b;
        }
    if (!finite) {
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++) {
                fc[UT(r, c)] = r == c ? P.nom[r] / P.floor : 0.0;
                fm[UT(r, c)] = r == c ? P.floor : 0.0;
            }
        dw = -1;
#pragma unroll
        for (int k = 0; k < 6; k++) ev[k] = (double)NAN;
    }
    // entry (r, c) of the output order, r <= c: out_order 1 swaps the two halves of the index range
    const bool sw = P.out_order == 1;
#define PUT(f, r, c) (sw ? f[((r) + 3) % 6 < ((c) + 3) % 6 ? UT(((r) + 3) % 6, ((c) + 3) % 6) : UT(((c) + 3) % 6, ((r) + 3) % 6)] : f[UT(r, c)])
    double* mine = lds + lane * MSTRIDE;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) {
            const double x = PUT(fc, r, c);
            mine[r * 6 + c] = x;
            mine[c * 6 + r] = x;
        }
    __syncthreads();
    flush_rows<36>(lds, cov + (size_t)base * 36, n, lane);
    if (active) deweighted[i] = dw;
    if (sqrt_info != nullptr) {     // (uniform)
        // R' = chol_upper(G) row by row, R = R' N^-1/2; G has its eigenvalues in [floor, 1]
        double g[21], R[21];
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++) g[UT(r, c)] = PUT(fm, r, c);
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double d = g[UT(j, j)];
#pragma unroll
            for (int k = 0; k < j; k++) d = fma(-R[UT(k, j)], R[UT(k, j)], d);
            const double rjj = sqrt(d);
            const double inv = 1.0 / rjj;
            R[UT(j, j)] = rjj;
#pragma unroll
            for (int c = j + 1; c < 6; c++) {
                double x = g[UT(j, c)];
#pragma unroll
                for (int k = 0; k < j; k++) x = fma(-R[UT(k, j)], R[UT(k, c)], x);
                R[UT(j, c)] = x * inv;
            }
        }
        __syncthreads();
        double* row = lds + lane * 21;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++) row[UT(r, c)] = R[UT(r, c)] * (sw ? P.is[(c + 3) % 6] : P.is[c]);
        __syncthreads();
        flush_rows<21>(lds, sqrt_info + (size_t)base * 21, n, lane);
    }
#undef PUT
    if (want_eig) {
        __syncthreads();
        double* row = lds + lane * 7;
#pragma unroll
        for (int k = 0; k < 6; k++) row[k] = ev[k];
        __syncthreads();
        flush_rows<6>(lds, eig + (size_t)base * 6, n, lane);
    }
}
#undef UT

int derr(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vf_set_last_error_(buf);
    return code;
}
#define HIPCHK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return derr(VF_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// launch() once and wait; if asked to, the time of one of `reps` further launches
template <typename Launch>
int run_timed(int reps, float* kernel_ms, Launch launch) {
    launch();
    HIPCHK(hipDeviceSynchronize());
    if (kernel_ms && reps > 0) {
        vf::Event e0, e1;
        HIPCHK(e0.ensure());
        HIPCHK(e1.ensure());
        HIPCHK(hipEventRecord(e0, 0));
        for (int r = 0; r < reps; r++) launch();
        HIPCHK(hipEventRecord(e1, 0));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *kernel_ms = ms / reps;
    }
    HIPCHK(hipGetLastError());
    return VF_OK;
}

// The batch entry points: upload `count` matrices (and poses, if given), launch(mats, poses, out) once and wait, time `reps`
// further launches if asked to, download `rows` rows of `count` values in equal shares to the host arrays of `outs`.
template <typename T, typename Launch>
int run_batch(const void* mats, const void* pose, int count, int rows, std::initializer_list<void*> outs, int reps, float* kernel_ms, Launch launch) {
    vf::DeviceBuf<T> d_m, d_p, d_o;
    const size_t mb = (size_t)count * 36 * sizeof(T), pb = (size_t)count * 6 * sizeof(T), ob = (size_t)rows / outs.size() * count * sizeof(T);
    HIPCHK(d_m.ensure(mb));
    HIPCHK(d_o.ensure(ob * outs.size()));
    HIPCHK(hipMemcpy(d_m, mats, mb, hipMemcpyHostToDevice));
    if (pose) {
        HIPCHK(d_p.ensure(pb));
        HIPCHK(hipMemcpy(d_p, pose, pb, hipMemcpyHostToDevice));
    }
    if (int rc = run_timed(reps, kernel_ms, [&]() { launch(d_m.get(), d_p.get(), d_o.get()); })) return rc;
    const char* from = (const char*)d_o.get();
    for (void* o : outs) {
        HIPCHK(hipMemcpy(o, from, ob, hipMemcpyDeviceToHost));
        from += ob;
    }
    return VF_OK;
}

// f(std::integral_constant<int, N>{}) for the block size of a subset (subset_off)
template <typename F>
void with_block(int subset, F&& f) {
    if (subset == 0) f(std::integral_constant<int, 6>{});
    else if (subset < 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 1>{});
}

// f(T{}) for the element type of a dtype id (checked by check_batch)
template <typename F>
int with_dtype(int dtype, F&& f) { return dtype == 0 ? f(double{}) : f(float{}); }

// one subset of one metric; metric = SPECTRUM: its three values, in the three arrays of `outs`
template <typename T>
int run_metric(const void* mats, const void* pose, int count, int subset, int metric, std::initializer_list<void*> outs, int reps, float* kernel_ms) {
    const int off = subset_off(subset);
    const dim3 grid((count + 63) / 64);
    return run_batch<T>(mats, pose, count, (int)outs.size(), outs, reps, kernel_ms, [&](const T* m, const T* p, T* o) {
        with_block(subset, [&](auto N) {
            if (metric == SPECTRUM) hipLaunchKernelGGL((k_degeneracy<T, N(), SPECTRUM>), grid, dim3(64), 0, 0, m, p, count, off, o);
            else with_metric(metric, [&](auto M) { hipLaunchKernelGGL((k_degeneracy<T, N(), M()>), grid, dim3(64), 0, 0, m, p, count, off, o); });
        });
    });
}

template <typename T>
int run_scores(const void* mats, const void* pose, int count, int metric, unsigned mask, void* out, int reps, float* kernel_ms) {
    const dim3 grid((count + 63) / 64);
    return run_batch<T>(mats, pose, count, __builtin_popcount(mask), {out}, reps, kernel_ms, [&](const T* m, const T* p, T* o) {
        with_metric(metric, [&](auto M) { hipLaunchKernelGGL((k_degeneracy_scores<T, M()>), grid, dim3(64), 0, 0, m, p, count, mask, o); });
    });
}

int check_subset(int subset) {
    if (subset < 0 || subset >= N_SUBSETS) return derr(VF_ERR_INVALID, "subset must be 0 (all), 1 (trans), 2 (rot) or 3 .. 8 (x y z roll pitch yaw)");
    return VF_OK;
}

int check_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return derr(VF_ERR_NO_DEVICE, "no HIP device visible; libvilfusion has no CPU path");
    return VF_OK;
}

// What the batch entry points refuse alike, in this order; *run: there are matrices, and a device to take them to
int check_batch(bool null_argument, int count, int metric, int dtype, bool has_pose, bool* run) {
    *run = false;
    if (null_argument || count < 0) return derr(VF_ERR_INVALID, "null argument");
    if (metric < 0 || metric >= N_METRICS) return derr(VF_ERR_INVALID, "unknown metric %d", metric);
    if (dtype != 0 && dtype != 1) return derr(VF_ERR_INVALID, "dtype must be 0 (f64) or 1 (f32)");
    if (metric_traits(metric).pose && !has_pose) return derr(VF_ERR_INVALID, "kullback_leibler needs poses");
    if (count == 0) return VF_OK;
    if (int rc = check_device()) return rc;
    *run = true;
    return VF_OK;
}

}  // namespace

// what vf_engine.hip reaches the windows kernel through (vf_kernels.hpp; not part of the ABI).  The caller has checked metric and mask.
namespace vf {
void launch_degeneracy_scores_windows(int metric, unsigned mask, const double* mats, const double* pose, const int* range, int B, int M,
                                      double* out, hipStream_t s) {
    with_metric(metric, [&](auto K) {
        hipLaunchKernelGGL((k_degeneracy_scores_windows<K()>), dim3((M + 63) / 64, B), dim3(64), 0, s, mats, pose, range, M, (size_t)B * M, mask, out);
    });
}
}  // namespace vf

extern "C" {

int vf_degeneracy_spectrum_batch(const void* mats, int count, int dtype, int subset, void* e_opt, void* max_eigen, void* condition_number,
                                 int reps, float* kernel_ms) {
    bool run;
    if (int rc = check_subset(subset)) return rc;
    if (int rc = check_batch(!mats || !e_opt || !max_eigen || !condition_number, count, E_OPT, dtype, false, &run); rc || !run) return rc;
    return with_dtype(dtype, [&](auto t) {
        return run_metric<decltype(t)>(mats, nullptr, count, subset, SPECTRUM, {e_opt, max_eigen, condition_number}, reps, kernel_ms);
    });
}

int vf_degeneracy_batch(const void* mats, const void* pose, int count, int dtype, int subset, int metric, void* out,
                        int reps, float* kernel_ms) {
    bool run;
    if (int rc = check_subset(subset)) return rc;
    if (int rc = check_batch(!mats || !out, count, metric, dtype, pose != nullptr, &run); rc || !run) return rc;
    return with_dtype(dtype, [&](auto t) { return run_metric<decltype(t)>(mats, pose, count, subset, metric, {out}, reps, kernel_ms); });
}

int vf_degeneracy_scores_batch(const void* mats, const void* pose, int count, int dtype, int metric, unsigned subset_mask, void* out,
                               int reps, float* kernel_ms) {
    bool run;
    if (subset_mask == 0 || (subset_mask >> N_SUBSETS) != 0) return derr(VF_ERR_INVALID, "subset_mask 0x%x: bits 0 .. 8, at least one", subset_mask);
    if (int rc = check_batch(!mats || !out, count, metric, dtype, pose != nullptr, &run); rc || !run) return rc;
    return with_dtype(dtype, [&](auto t) { return run_scores<decltype(t)>(mats, pose, count, metric, subset_mask, out, reps, kernel_ms); });
}

int vf_dopt_filter_f32(const float* hessians, int count, float rot_thr, float trans_thr, float* rot_dopt,
                       float* trans_dopt, unsigned char* keep) {
    if (!hessians || !rot_dopt || !trans_dopt || !keep || count < 0) return derr(VF_ERR_INVALID, "null argument");
    if (count == 0) return VF_OK;
    if (int rc = check_device()) return rc;
    vf::DeviceBuf<float> d_h, d_r, d_t;
    vf::DeviceBuf<unsigned char> d_k;
    HIPCHK(d_h.ensure((size_t)count * 36 * sizeof(float)));
    HIPCHK(d_r.ensure(count * sizeof(float)));
    HIPCHK(d_t.ensure(count * sizeof(float)));
    HIPCHK(d_k.ensure(count));
    HIPCHK(hipMemcpy(d_h, hessians, (size_t)count * 36 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_dopt_filter, dim3((count + 255) / 256), dim3(256), 0, 0, d_h.get(), count, rot_thr, trans_thr, d_r.get(), d_t.get(), d_k.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(rot_dopt, d_r, count * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(trans_dopt, d_t, count * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(keep, d_k, count, hipMemcpyDeviceToHost));
    return VF_OK;
}

int vf_degeneracy_remap_batch(const void* hessians36, int count, int dtype, const double nom6[6], double trans_thr, double rot_thr,
                              double floor, int out_order, double* cov36, double* sqrt_info21, double* eig6, int32_t* deweighted,
                              int reps, float* kernel_ms) {
    if (!hessians36 || !nom6 || !cov36 || !deweighted || count < 0) return derr(VF_ERR_INVALID, "null argument");
    if (dtype != 0 && dtype != 1) return derr(VF_ERR_INVALID, "dtype must be 0 (f64) or 1 (f32)");
    if (out_order != 0 && out_order != 1) return derr(VF_ERR_INVALID, "out_order must be 0 (input order) or 1 ([rot, trans])");
    if (!(trans_thr > 0.0) || !(rot_thr > 0.0) || !std::isfinite(trans_thr) || !std::isfinite(rot_thr))
        return derr(VF_ERR_INVALID, "eigenvalue thresholds must be positive and finite (trans %g, rot %g)", trans_thr, rot_thr);
    if (!(floor > 0.0 && floor <= 1.0)) return derr(VF_ERR_INVALID, "floor %g: must lie in (0, 1]", floor);
    for (int k = 0; k < 6; k++)
        if (!(nom6[k] > 0.0) || !std::isfinite(nom6[k])) return derr(VF_ERR_INVALID, "nom6[%d] = %g: the nominal covariance must be positive and finite", k, nom6[k]);
    if (count == 0) return VF_OK;
    if (int rc = check_device()) return rc;
    RemapParams P;
    for (int k = 0; k < 6; k++) {
        P.d[k] = 1.0 / std::sqrt(k < 3 ? trans_thr : rot_thr);
        P.nom[k] = nom6[k];
        P.s[k] = std::sqrt(nom6[k]);
        P.is[k] = 1.0 / std::sqrt(nom6[k]);
    }
    P.floor = floor;
    P.out_order = out_order;
    const size_t n = (size_t)count, esz = dtype == 0 ? sizeof(double) : sizeof(float);
    vf::DeviceBuf<char> d_h;
    vf::DeviceBuf<double> d_c, d_r, d_e;
    vf::DeviceBuf<int> d_w;
    HIPCHK(d_h.ensure(n * 36 * esz));
    HIPCHK(d_c.ensure(n * 36 * sizeof(double)));
    if (sqrt_info21) HIPCHK(d_r.ensure(n * 21 * sizeof(double)));
    if (eig6) HIPCHK(d_e.ensure(n * 6 * sizeof(double)));
    HIPCHK(d_w.ensure(n * sizeof(int)));
    HIPCHK(hipMemcpy(d_h, hessians36, n * 36 * esz, hipMemcpyHostToDevice));
    const dim3 grid((count + 63) / 64);
    if (int rc = run_timed(reps, kernel_ms, [&]() {
            if (dtype == 0) hipLaunchKernelGGL((k_remap_covariance<double>), grid, dim3(64), 0, 0, (const double*)d_h.get(), count, P, d_c.get(), d_r.get(), d_e.get(), d_w.get());
            else hipLaunchKernelGGL((k_remap_covariance<float>), grid, dim3(64), 0, 0, (const float*)d_h.get(), count, P, d_c.get(), d_r.get(), d_e.get(), d_w.get());
        })) return rc;
    HIPCHK(hipMemcpy(cov36, d_c, n * 36 * sizeof(double), hipMemcpyDeviceToHost));
    if (sqrt_info21) HIPCHK(hipMemcpy(sqrt_info21, d_r, n * 21 * sizeof(double), hipMemcpyDeviceToHost));
    if (eig6) HIPCHK(hipMemcpy(eig6, d_e, n * 6 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(deweighted, d_w, n * sizeof(int), hipMemcpyDeviceToHost));
    return VF_OK;
}

}  // extern "C"
