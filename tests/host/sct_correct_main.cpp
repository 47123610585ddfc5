// The corrected count of mi_prep_sct_correct (mi_sct::corrected_count, csrc/mi_sct_math.h: the text every kernel form calls)
// as a host program: reads lines of `x mu alpha mu_r` (hexadecimal or decimal floats) from stdin and prints, for each, the
// corrected count as a hexadecimal float and whether the value before rounding was finite.
// tests/test_sct_correct_host.py compares them with the numpy restatement (tests/sct_correct_reference.py).
#include <cstdio>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_sct_math.h"

int main()
{
    double x, mu, alpha, mu_r;
    while (std::scanf("%la %la %la %la", &x, &mu, &alpha, &mu_r) == 4) {
        bool finite = false;
        const double c = mi_sct::corrected_count(x, mu, alpha, mu_r, mi_sct::nb_sd(mu_r, alpha), &finite);
        std::printf("%a %d\n", c, finite ? 1 : 0);
    }
    return 0;
}
