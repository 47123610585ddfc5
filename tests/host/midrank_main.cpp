// Stand-alone host program over the pure parts of csrc/mi_midrank.h: the tie-run search against a linear scan, the
// order-preserving key, the zero test, the power of two of the sort, and the index arithmetic of the bitonic network
// (sort_pair, the text wg_sort_u64 compiles) run serially over t for every pass.
// Built with -fsanitize=address,undefined by tests/test_midrank_host.py; prints "ok" and a count of checks, returns 0.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_midrank.h"

using namespace mi_midrank;
typedef unsigned long long u64;

static long checks = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        ++checks;                                                                       \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

static uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// exactly nnz entries (tie_run may read none past them): keys in the high word, distinct ids in the low word
static std::vector<u64> entries(const std::vector<uint32_t> &keys)
{
    std::vector<u64> S(keys.size());
    for (size_t p = 0; p < keys.size(); ++p) S[p] = ((u64)keys[p] << 32) | (uint32_t)(keys.size() - p);
    return S;
}

static void check_tie_run(const std::vector<uint32_t> &keys, int p)
{
    const std::vector<u64> S = entries(keys);
    const int nnz = (int)keys.size();
    int lo = p, hi = p + 1;
    while (lo > 0 && keys[lo - 1] == keys[p]) --lo;
    while (hi < nnz && keys[hi] == keys[p]) ++hi;
    int glo = -1, ghi = -1;
    tie_run(S.data(), p, nnz, &glo, &ghi);
    CHECK(glo == lo && ghi == hi);
}

static void test_tie_run()
{
    // every non-decreasing sequence of length 1 .. 12 over 4 key values, every position
    for (int len = 1; len <= 12; ++len)
        for (int a = 0; a <= len; ++a)
            for (int b = a; b <= len; ++b)
                for (int c = b; c <= len; ++c) {                                         // key 0 on [0, a), 1 on [a, b), 2 on [b, c), 3 after
                    std::vector<uint32_t> keys(len);
                    for (int p = 0; p < len; ++p) keys[p] = 0x7ffffffeu + (uint32_t)((p >= a) + (p >= b) + (p >= c));
                    for (int p = 0; p < len; ++p) check_tie_run(keys, p);
                }
    // 5000 entries in runs of 1, 2 and 4097, both ends of every run
    std::vector<uint32_t> keys;
    std::vector<int> starts;
    const int runs[] = {1, 2, 4097, 2, 1, 1, 2};
    uint32_t key = 5u;
    for (size_t r = 0; keys.size() < 5000; ++r) {
        int len = runs[r % 7];
        if (keys.size() + len > 5000) len = (int)(5000 - keys.size());
        starts.push_back((int)keys.size());
        keys.insert(keys.end(), len, key);
        key += 1u + (uint32_t)(r % 3) * 0x10000000u;
    }
    CHECK(keys.size() == 5000 && std::is_sorted(keys.begin(), keys.end()));
    starts.push_back(5000);
    for (size_t r = 0; r + 1 < starts.size(); ++r) {
        check_tie_run(keys, starts[r]);
        check_tie_run(keys, starts[r + 1] - 1);
    }
}

static void test_keys()
{
    const float pos[] = {FLT_TRUE_MIN, FLT_MIN, 1.0f, nextafterf(1.0f, 2.0f), FLT_MAX};
    std::vector<float> v;
    for (int i = 4; i >= 0; --i) v.push_back(-pos[i]);
    for (int i = 0; i < 5; ++i) v.push_back(pos[i]);
    CHECK(std::is_sorted(v.begin(), v.end()));
    for (size_t i = 0; i < v.size(); ++i) {
        const uint32_t k = order_key(bits_of(v[i]));
        CHECK(!zero_bits(bits_of(v[i])));
        CHECK(k != 0xffffffffu);
        CHECK((v[i] < 0.0f) == (k < 0x80000000u));
        CHECK(k == order_key(bits_of(v[i] * 1.0f)));                                     // equal floats, equal keys
        if (i > 0) CHECK(order_key(bits_of(v[i - 1])) < k);
    }
    CHECK(zero_bits(bits_of(0.0f)) && zero_bits(bits_of(-0.0f)) && bits_of(-0.0f) == 0x80000000u);
    CHECK(!zero_bits(bits_of(FLT_TRUE_MIN)) && !zero_bits(bits_of(-FLT_TRUE_MIN)) && bits_of(FLT_TRUE_MIN) == 1u);
}

static void test_pow2()
{
    CHECK(pow2_at_least(0) == 0 && pow2_at_least(1) == 1 && pow2_at_least(2) == 2 && pow2_at_least(3) == 4);
    for (int k = 2; k <= 20; ++k) {
        const int v = 1 << k;
        CHECK(pow2_at_least(v - 1) == v && pow2_at_least(v) == v && pow2_at_least(v + 1) == 2 * v);
    }
}

// wg_sort_u64 with its threads run one after another: within a pass the pairs are disjoint, so the order is free
static void serial_sort(std::vector<u64> &S)
{
    const int P = (int)S.size();
    std::vector<char> seen(S.size());
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            std::fill(seen.begin(), seen.end(), 0);
            for (int t = 0; t < (P >> 1); ++t) {
                int lo, hi;
                const bool up = sort_pair(t, k, j, &lo, &hi);
                CHECK(lo >= 0 && lo < hi && hi < P && !seen[lo] && !seen[hi]);           // every entry in exactly one pair
                seen[lo] = seen[hi] = 1;
                const u64 x = S[lo], y = S[hi];
                if ((x > y) == up) {
                    S[lo] = y;
                    S[hi] = x;
                }
            }
        }
}

static void test_network()
{
    std::vector<u64> perm(8);
    for (int i = 0; i < 8; ++i) perm[i] = ((u64)(0x80000000u + 3u * (uint32_t)i) << 32) | (uint32_t)(7 - i);
    std::vector<u64> sorted = perm;
    do {
        std::vector<u64> S = perm;
        serial_sort(S);
        CHECK(S == sorted);
    } while (std::next_permutation(perm.begin(), perm.end()));
    std::mt19937_64 gen(20);
    for (int P = 1; P <= 8192; P <<= 1)
        for (int rep = 0; rep < 3; ++rep) {
            const int nnz = rep == 0 ? P : rep == 1 ? P / 2 + 1 : (int)(gen() % (u64)P) + 1;      // the rest is ~0 pads
            std::vector<u64> S(P, ~0ull);
            for (int p = 0; p < nnz; ++p) S[p] = ((u64)(uint32_t)(gen() % 97u + 1u) << 32) | (uint32_t)p;      // tied keys, unique words
            std::vector<u64> want = S;
            std::sort(want.begin(), want.end());
            serial_sort(S);
            CHECK(S == want);
            for (int p = nnz; p < P; ++p) CHECK(S[p] == ~0ull);
        }
    std::vector<u64> none;
    serial_sort(none);                                                                   // P = 0: no pass
}

int main()
{
    test_tie_run();
    test_keys();
    test_pow2();
    test_network();
    printf("ok %ld checks\n", checks);
    return 0;
}
