// Stand-alone host program over csrc/mi_prep_csr.h, the HIP-free half of a sparse mi_prep_matrix: every cause of
// MI_EINVAL / MI_EUNSUPPORTED of mi_prep_create_csr_f32 on its own, the shapes at the edges (no entry at all, empty rows
// and columns, g = 1, a full row, stored zeros), and the transpose of random matrices against a brute-force one.  Built
// with -fsanitize=address,undefined by tests/test_prep_sparse_host.py; prints "ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_prep_csr.h"

using namespace mi_prep_csr;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

struct Csr {
    int n = 0, g = 0;
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<float> data;
};

static const int kMaxCells = 1 << 23;
static const int64_t kMaxNnz = 2147483647ll;

static int check_of(const Csr &m, const char *needle, int max_cells = kMaxCells, int64_t max_nnz = kMaxNnz)
{
    char msg[160];
    memset(msg, 'x', sizeof msg);
    const int rc = check(m.indptr.data(), m.indices.data(), m.data.data(), m.n, m.g, max_cells, max_nnz, msg, sizeof msg);
    CHECK(memchr(msg, 0, sizeof msg) != nullptr);
    if (rc == kOk) CHECK(msg[0] == 0);
    else if (!strstr(msg, needle)) {
        fprintf(stderr, "message '%s' lacks '%s'\n", msg, needle);
        exit(1);
    }
    return rc;
}

// 3 cells x 4 genes: row 0 = {0: 1, 2: 2}, row 1 empty, row 2 = {1: 3, 2: 0 (stored), 3: 5}; gene 0 .. 3 hold 1, 1, 2, 1
static Csr small()
{
    Csr m;
    m.n = 3; m.g = 4;
    m.indptr = {0, 2, 2, 5};
    m.indices = {0, 2, 1, 2, 3};
    m.data = {1.0f, 2.0f, 3.0f, 0.0f, 5.0f};
    return m;
}

// xorshift: the program must not depend on the C library's generator
static uint32_t rng_state = 2463534242u;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

static Csr random_csr(int n, int g, uint32_t keep_of_256)
{
    Csr m;
    m.n = n; m.g = g;
    m.indptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < g; ++j)
            if ((rnd() & 255u) < keep_of_256) {
                m.indices.push_back(j);
                m.data.push_back((rnd() & 7u) == 0 ? 0.0f : (float)(1 + (rnd() & 15u)));      // one in eight a stored zero
            }
        m.indptr.push_back((int64_t)m.indices.size());
    }
    return m;
}

static void check_transpose(const Csr &m)
{
    CHECK(check_of(m, "") == kOk);
    std::vector<int64_t> colptr;
    std::vector<int32_t> rows, pos;
    transpose(m.indptr.data(), m.indices.data(), m.n, m.g, colptr, rows, pos);
    const size_t nnz = m.indices.size();
    CHECK(colptr.size() == (size_t)m.g + 1 && rows.size() == nnz && pos.size() == nnz);
    CHECK(colptr[0] == 0 && colptr[(size_t)m.g] == (int64_t)nnz);
    // brute force: column j's entries are the (row, position) pairs of every CSR entry with that column, rows ascending
    size_t k = 0;
    for (int j = 0; j < m.g; ++j) {
        CHECK(colptr[(size_t)j] == (int64_t)k);
        for (int i = 0; i < m.n; ++i)
            for (int64_t e = m.indptr[(size_t)i]; e < m.indptr[(size_t)i + 1]; ++e)
                if (m.indices[(size_t)e] == j) {
                    CHECK(k < nnz && rows[k] == i && pos[k] == (int32_t)e);
                    ++k;
                }
    }
    CHECK(k == nnz);
    std::vector<char> seen(nnz, 0);                                // pos is a permutation
    for (size_t q = 0; q < nnz; ++q) {
        CHECK(pos[q] >= 0 && (size_t)pos[q] < nnz && !seen[(size_t)pos[q]]);
        seen[(size_t)pos[q]] = 1;
    }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    CHECK(check_of(small(), "") == kOk);

    // ---- every cause of MI_EINVAL, each on its own -------------------------------------------------------------------------
    {
        const Csr m = small();
        char msg[160];
        CHECK(check(nullptr, m.indices.data(), m.data.data(), 3, 4, kMaxCells, kMaxNnz, msg, sizeof msg) == kEinval && strstr(msg, "NULL"));
        CHECK(check(m.indptr.data(), nullptr, m.data.data(), 3, 4, kMaxCells, kMaxNnz, msg, sizeof msg) == kEinval && strstr(msg, "NULL"));
        CHECK(check(m.indptr.data(), m.indices.data(), nullptr, 3, 4, kMaxCells, kMaxNnz, msg, sizeof msg) == kEinval && strstr(msg, "NULL"));
        CHECK(check(m.indptr.data(), m.indices.data(), m.data.data(), 3, 4, kMaxCells, kMaxNnz, nullptr, 0) == kOk);   // no room for a text
    }
    { Csr m = small(); m.n = 1; CHECK(check_of(m, "n must be") == kEinval); }
    { Csr m = small(); m.g = 0; CHECK(check_of(m, "g must be") == kEinval); }
    { Csr m = small(); m.indptr[0] = 1; CHECK(check_of(m, "indptr[0]") == kEinval); }
    { Csr m = small(); m.indptr[2] = 1; CHECK(check_of(m, "decreases") == kEinval); }
    { Csr m = small(); m.indices[4] = 4; CHECK(check_of(m, "outside") == kEinval); }
    { Csr m = small(); m.indices[0] = -1; CHECK(check_of(m, "outside") == kEinval); }
    { Csr m = small(); m.indices[3] = 1; CHECK(check_of(m, "ascending") == kEinval); }              // a repeated column
    { Csr m = small(); m.indices[2] = 2; m.indices[3] = 1; CHECK(check_of(m, "ascending") == kEinval); }   // a descending pair
    { Csr m = small(); m.data[1] = nan; CHECK(check_of(m, "NaN") == kEinval); }
    { Csr m = small(); m.data[1] = inf; CHECK(check_of(m, "NaN") == kEinval); }
    { Csr m = small(); m.data[1] = -1.0f; CHECK(check_of(m, "NaN") == kEinval); }
    { Csr m = small(); m.data[1] = -0.0f; CHECK(check_of(m, "") == kOk); }                         // -0 >= 0: as the dense entry
    // ---- ... and of MI_EUNSUPPORTED ----------------------------------------------------------------------------------------
    CHECK(check_of(small(), "cells exceed", 2) == kEunsupported);
    CHECK(check_of(small(), "stored entries exceed", kMaxCells, 4) == kEunsupported);
    CHECK(check_of(small(), "", 3, 5) == kOk);

    // ---- edge shapes -------------------------------------------------------------------------------------------------------
    {
        Csr m;                                                     // no entry at all (the vectors' data() may be null: one element)
        m.n = 5; m.g = 7;
        m.indptr.assign(6, 0);
        m.indices.assign(1, 0);
        m.data.assign(1, 0.0f);
        char msg[160];
        CHECK(check(m.indptr.data(), m.indices.data(), m.data.data(), m.n, m.g, kMaxCells, kMaxNnz, msg, sizeof msg) == kOk);
        std::vector<int64_t> colptr;
        std::vector<int32_t> rows, pos;
        transpose(m.indptr.data(), m.indices.data(), m.n, m.g, colptr, rows, pos);
        CHECK(colptr == std::vector<int64_t>(8, 0) && rows.empty() && pos.empty());
    }
    check_transpose(small());                                      // an empty row, a stored zero
    {
        Csr m = small();                                           // ... and an empty column (gene 3 of 5), first and last rows empty
        m.n = 5; m.g = 6;
        m.indptr = {0, 0, 2, 2, 5, 5};
        m.indices = {0, 2, 1, 2, 5};
        check_transpose(m);
    }
    {
        Csr m;                                                     // g = 1
        m.n = 4; m.g = 1;
        m.indptr = {0, 1, 1, 2, 3};
        m.indices = {0, 0, 0};
        m.data = {2.0f, 0.0f, 7.0f};
        check_transpose(m);
    }
    {
        Csr m;                                                     // a full row between two empty ones
        m.n = 3; m.g = 130;
        m.indptr = {0, 0, 130, 130};
        for (int j = 0; j < 130; ++j) { m.indices.push_back(j); m.data.push_back((float)(j + 1)); }
        check_transpose(m);
    }
    // ---- random matrices, stored zeros included ----------------------------------------------------------------------------
    check_transpose(random_csr(2, 1, 128));
    check_transpose(random_csr(65, 130, 77));
    check_transpose(random_csr(257, 63, 5));                       // 2 %: empty rows and columns
    check_transpose(random_csr(40, 300, 255));                     // nearly full
    printf("ok\n");
    return 0;
}
