// tests/native/robust_scalars.cpp -- alpha and gamma of the robust losses (vil_sensor_fusion_amd/csrc/vf_robust.hpp) on the CPU,
// against references computed at 50 digits (tests/test_robust_host.py writes them with mpmath).
//
// usage: robust_scalars <file> <bar>
// Every line of <file> is one grid point:  loss  s  k  alpha_hi alpha_lo  gamma_hi gamma_lo   (hex floats; a reference is the sum
// of its two doubles, 106 bits, compared in long double).  Huber points have s > k: s <= k is the caller's pass-through, for
// which the program checks what the sink relies on instead -- that `s <= k` is true at s = k and false for a NaN.  Prints the
// largest relative error per loss and function; exit status 1 if one exceeds <bar> or a value is not finite.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "vf_robust.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: robust_scalars <file> <bar>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const long double bar = strtold(argv[2], nullptr);
    long double worst[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    int failures = 0, points = 0, loss;
    double s, k, ah, al, gh, gl;
    while (fscanf(f, "%d %la %la %la %la %la %la", &loss, &s, &k, &ah, &al, &gh, &gl) == 7) {
        if (loss < vf::LOSS_HUBER || loss > vf::LOSS_GEMAN_MCCLURE || (loss == vf::LOSS_HUBER && !(s > k))) { printf("FAILED bad grid point\n"); return 2; }
        points++;
        const double got[2] = {vf::robust_alpha(loss, s, k), vf::robust_gamma(loss, s, k)};
        const long double want[2] = {(long double)ah + (long double)al, (long double)gh + (long double)gl};
        for (int q = 0; q < 2; q++) {
            long double err;
            if (!std::isfinite(got[q])) err = INFINITY;
            else if (want[q] == 0.0L) err = got[q] == 0.0 ? 0.0L : INFINITY;
            else err = fabsl(((long double)got[q] - want[q]) / want[q]);
            if (err > worst[loss][q]) worst[loss][q] = err;
            if (!(err <= bar)) {
                failures++;
                printf("FAILED loss %d %s at s = %a, k = %a: got %a, relative error %.3Le > %.3Le\n", loss, q ? "gamma" : "alpha", s, k, got[q], err, bar);
            }
        }
    }
    fclose(f);
    // s = 0 exactly: r^ = 0 and J^ = J need alpha = 1 and a finite gamma
    for (int l = vf::LOSS_CAUCHY; l <= vf::LOSS_GEMAN_MCCLURE; l++)
        if (vf::robust_alpha(l, 0.0, 0.7) != 1.0 || !std::isfinite(vf::robust_gamma(l, 0.0, 0.7))) { failures++; printf("FAILED loss %d at s = 0\n", l); }
    if (vf::robust_gamma(vf::LOSS_CAUCHY, 0.0, 0.5) != -2.0 || vf::robust_gamma(vf::LOSS_GEMAN_MCCLURE, 0.0, 0.5) != -4.0) { failures++; printf("FAILED gamma(0) is not -1 / (2 k^2) resp. -1 / k^2\n"); }
    // a norm that is not finite must not come out finite
    const double bad[3] = {NAN, INFINITY, -NAN};
    for (int l = vf::LOSS_HUBER; l <= vf::LOSS_GEMAN_MCCLURE; l++)
        for (double x : bad) {
            const double a = vf::robust_alpha(l, x, 1.5) * x;        // what r^ = alpha r is made of
            if (std::isfinite(a)) { failures++; printf("FAILED loss %d: alpha(%g) * %g = %g is finite\n", l, x, x, a); }
        }
    { const double kk = 1.345, nan = NAN; if (!(kk <= kk) || (nan <= kk)) { failures++; printf("FAILED the inlier test\n"); } }
    const char* names[4] = {"", "huber", "cauchy", "geman_mcclure"};
    for (int l = 1; l <= 3; l++) printf("max relative error %-14s alpha %.3Le gamma %.3Le\n", names[l], worst[l][0], worst[l][1]);
    if (failures) { printf("robust_scalars: %d failure(s)\n", failures); return 1; }
    printf("robust_scalars ok (%d points)\n", points);
    return 0;
}
