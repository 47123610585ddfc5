// The digamma and trigamma functions of the negative-binomial fit (csrc/mi_sct_math.h) as a host program: prints, for
// `count` arguments spaced evenly in log10 over [1e-30, 1e30], the argument and both values as hexadecimal floats, one line each.
// tests/test_sct_host.py compares them with scipy.special.
#include <cstdio>
#include <cstdlib>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_sct_math.h"

int main(int argc, char **argv)
{
    const int count = argc > 1 ? std::atoi(argv[1]) : 2001;
    if (count < 2) return 2;
    for (int k = 0; k < count; ++k) {
        const double x = pow(10.0, -30.0 + 60.0 * (double)k / (double)(count - 1));
        std::printf("%a %a %a\n", x, mi_sct::digamma(x), mi_sct::trigamma(x));
    }
    return 0;
}
