// vf_robust.hpp -- the scalar functions of a robust loss on a whitened residual of norm s, in its square-root form:
//     alpha(s) = sqrt(2 rho(s)) / s        gamma(s) = alpha'(s) / s
// so that r^ = alpha r has 0.5 |r^|^2 = rho(s) exactly and J^ = (alpha I + gamma r r^T) J is its Jacobian (DESIGN.md "4i").
// Conventions of GTSAM's mEstimator classes, k > 0 the parameter, u = s^2 / k^2:
//     Huber          rho = s^2 / 2 (s <= k),  k (s - k / 2) (s > k)
//     Cauchy         rho = (k^2 / 2) log(1 + u)
//     Geman-McClure  rho = (1 / 2) k^2 s^2 / (k^2 + s^2)
// Host and device code, nothing else in here (tests/native/robust_scalars.cpp checks it on the CPU against 50 digits).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VF_HD __host__ __device__ inline
#else
#define VF_HD inline
#endif

namespace vf {

constexpr int LOSS_NONE = 0, LOSS_HUBER = 1, LOSS_CAUCHY = 2, LOSS_GEMAN_MCCLURE = 3;     // VF_LOSS_*

// Huber: the caller decides inlier / outlier (s <= k is a pass-through that touches no word); these are the s > k branch.
// d = s - k is exact up to 2 k (Sterbenz) and 2 s - k = s + d has no cancellation.
VF_HD double huber_alpha(double s, double k) { return sqrt(k * (s + (s - k))) / s; }
VF_HD double huber_gamma(double s, double k) {
    const double d = s - k;
    return -(k / s) * (d / s) / (s * sqrt(k * (s + d)));
}

VF_HD double cauchy_alpha(double s, double k) {
    const double t = s / k, u = t * t;
    return u > 0.0 ? sqrt(log1p(u) / u) : (u == 0.0 ? 1.0 : u);     // (u < 0 never; NaN goes through)
}
// gamma = g(u) / (alpha k^2), g(u) = (u / (1 + u) - log1p(u)) / u^2 = -1/2 + 2 u / 3 - 3 u^2 / 4 + ...: the two terms cancel to
// u^2 / 2, a relative error of 2 eps / u.  Up to u = 1 the form without a cancellation: with z = u / (2 + u) <= 1 / 3,
// log1p(u) = 2 atanh(z) and u / (1 + u) = 2 z / (1 + z), so
//     g(u) = -(1 - z)^2 / 2 * [1 / (1 + z) + z (1/3 + z^2 / 5 + z^4 / 7 + ...)],
// every term positive; 9^-18 < 2^-56 ends the series.  Above u = 1 the difference keeps all but 3 bits.
VF_HD double cauchy_g(double u) {
    if (u <= 1.0) {
        const double z = u / (2.0 + u), z2 = z * z;
        double t = 1.0 / 37.0;
        for (int n = 16; n >= 0; n--) t = t * z2 + 1.0 / (double)(2 * n + 3);
        const double w = 1.0 - z;
        return -0.5 * w * w * (1.0 / (1.0 + z) + z * t);
    }
    return (u / (1.0 + u) - log1p(u)) / (u * u);
}
VF_HD double cauchy_gamma(double s, double k) {
    const double t = s / k, u = t * t;
    const double a = u > 0.0 ? sqrt(log1p(u) / u) : (u == 0.0 ? 1.0 : u);
    return cauchy_g(u) / (a * k) / k;
}

// (a norm that is not finite -- an infinite residual, or a finite one beyond 1e154 whose sum of squares has overflowed -- must not
// give alpha = 0 and with it a silently finite r^ = 0: inf - inf is the NaN that reaches the cost and the `nonfinite` counts)
VF_HD double gm_alpha(double s, double k) {
    const double t = s / k, w = 1.0 + t * t;
    return w < INFINITY ? 1.0 / sqrt(w) : w - w;
}
VF_HD double gm_gamma(double s, double k) {
    const double t = s / k, w = 1.0 + t * t;
    return -1.0 / (w * sqrt(w) * k) / k;
}

// by loss id (Huber: s > k)
VF_HD double robust_alpha(int loss, double s, double k) {
    return loss == LOSS_HUBER ? huber_alpha(s, k) : loss == LOSS_CAUCHY ? cauchy_alpha(s, k) : gm_alpha(s, k);
}
VF_HD double robust_gamma(int loss, double s, double k) {
    return loss == LOSS_HUBER ? huber_gamma(s, k) : loss == LOSS_CAUCHY ? cauchy_gamma(s, k) : gm_gamma(s, k);
}

}  // namespace vf
