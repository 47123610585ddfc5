// mi_sct_math.h -- the scalar functions of SCTransform in fp64.  The corrected count of mi_prep_sct_correct (every kernel
// form of csrc/prep_kernels.hip, dense or sparse, stored entry or zero, calls corrected_count below; the host program is
// tests/host/sct_correct_main.cpp).  The digamma and trigamma functions of the negative-binomial fit (k_sct_nb_fit),
// for x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x (psi'(x) = psi'(x + 1) + 1 / x^2) up to an argument >= 8,
// then the asymptotic series with the Bernoulli numbers through B16 (psi) and B18 (psi'), whose first omitted term is below
// 2e-16 of the value at 8.  Plain C++: the device code and a host program (tests/host/sct_psi_main.cpp) compile the same
// text; every operation is a separate multiply, add or divide.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MI_SCT_FN __host__ __device__ __forceinline__
#else
#define MI_SCT_FN inline
#endif

namespace mi_sct {

MI_SCT_FN double digamma(double x)
{
    double r = 0.0;
    while (x < 8.0) {
        r = r - 1.0 / x;
        x = x + 1.0;
    }
    const double i = 1.0 / x, i2 = i * i;
    // sum_k B_2k / (2k x^2k), k = 1 .. 8, by Horner in 1 / x^2
    double s = 3617.0 / 8160.0;
    s = -1.0 / 12.0 + i2 * s;
    s = 691.0 / 32760.0 + i2 * s;
    s = -1.0 / 132.0 + i2 * s;
    s = 1.0 / 240.0 + i2 * s;
    s = -1.0 / 252.0 + i2 * s;
    s = 1.0 / 120.0 + i2 * s;
    s = -1.0 / 12.0 + i2 * s;
    return r + ((log(x) - 0.5 * i) + i2 * s);
}

MI_SCT_FN double trigamma(double x)
{
    double r = 0.0;
    while (x < 8.0) {
        r = r + 1.0 / (x * x);
        x = x + 1.0;
    }
    const double i = 1.0 / x, i2 = i * i;
    // sum_k B_2k / x^(2k + 1), k = 1 .. 9, by Horner in 1 / x^2
    double s = 43867.0 / 798.0;
    s = -3617.0 / 510.0 + i2 * s;
    s = 7.0 / 6.0 + i2 * s;
    s = -691.0 / 2730.0 + i2 * s;
    s = 5.0 / 66.0 + i2 * s;
    s = -1.0 / 30.0 + i2 * s;
    s = 1.0 / 42.0 + i2 * s;
    s = -1.0 / 30.0 + i2 * s;
    s = 1.0 / 6.0 + i2 * s;
    return r + (i + i2 * (0.5 + i * s));
}

// the standard deviation of the negative-binomial model at mean mu: sqrt(mu + alpha mu^2)
MI_SCT_FN double nb_sd(double mu, double alpha) { return sqrt(mu + alpha * (mu * mu)); }

// The corrected count of x: its Pearson residual under (mu, alpha), unclipped, carried to the reference depth's mean mu_r
// and standard deviation s_r = nb_sd(mu_r, alpha), rounded half to even, not below 0 (a separate multiply and add).
// *finite: is mu_r + r s_r finite -- an overflowed or vanished mu gives an infinity or a NaN, which the maximum would hide.
MI_SCT_FN double corrected_count(double x, double mu, double alpha, double mu_r, double s_r, bool *finite)
{
    const double r = (x - mu) / nb_sd(mu, alpha);
    const double v = mu_r + r * s_r;
    *finite = v - v == 0.0;
    const double c = rint(v);
    return c > 0.0 ? c : 0.0;                                     // fmax(c, 0.0), with +0.0 for -0.0 (and for a NaN)
}

}  // namespace mi_sct
