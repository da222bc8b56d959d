/* CPU check of the bin-edge request's validator (lcmap-firebird_amd/csrc/ccdgpu_checks.cpp): a
 * stand-alone program, built with -fsanitize=address,undefined and run by
 * tests/test_randomforest_splits.py.  ccdgpu_splits_check on rows given in a heap block of exactly
 * their size, so a read past it is a sanitizer error: the accepted edge cases and every rejection. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../include/ccdgpu.h"

#define REQUIRE(cond, what)                                                                 \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::printf("%s:%d: %s (%s) -- %s\n", __FILE__, __LINE__, what, #cond, ccdgpu_last_error()); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

static bool refused(int rc, const char *needle) { return rc == CCDGPU_EINVAL && std::strstr(ccdgpu_last_error(), needle); }

static int checks() {
    // 5 rows of 3 features in a heap block of exactly that size
    const int64_t n_rows = 5;
    const int32_t nf = 3;
    double *x = (double *)std::malloc(sizeof(double) * n_rows * nf);
    for (int64_t i = 0; i < n_rows * nf; ++i) x[i] = (double)i * 0.5 - 3.0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    REQUIRE(ccdgpu_splits_check(x, n_rows, nf, 32) == 0, "a good request");
    REQUIRE(ccdgpu_splits_check(x, 1, nf, 2) == 0, "one row, two bins");
    REQUIRE(ccdgpu_splits_check(x, n_rows, nf, CCDGPU_TRAIN_MAX_EDGES + 1) == 0, "64 bins");
    REQUIRE(ccdgpu_splits_check(x, 1, (int32_t)(n_rows * nf), 32) == 0, "one row of 15 features: the same block");
    REQUIRE(ccdgpu_splits_check(nullptr, 0, nf, 32) == 0, "no rows: x may be NULL");
    REQUIRE(ccdgpu_splits_check(x, 0, nf, 32) == 0, "no rows");
    x[0] = -0.0, x[1] = 5e-324, x[2] = -1.7e308, x[3] = std::numeric_limits<double>::max();
    REQUIRE(ccdgpu_splits_check(x, n_rows, nf, 32) == 0, "zeros, a denormal and the largest doubles are finite");
    // NULL
    REQUIRE(refused(ccdgpu_splits_check(nullptr, n_rows, nf, 32), "x is NULL"), "NULL x");
    // counts (refused before x is read: the block is too small for these sizes)
    REQUIRE(refused(ccdgpu_splits_check(x, -1, nf, 32), "n_rows"), "negative rows");
    REQUIRE(refused(ccdgpu_splits_check(x, CCDGPU_TRAIN_MAX_ROWS + 1, nf, 32), "n_rows"), "too many rows");
    REQUIRE(refused(ccdgpu_splits_check(x, n_rows, 0, 32), "n_features"), "no features");
    REQUIRE(refused(ccdgpu_splits_check(x, n_rows, CCDGPU_FOREST_MAX_FEATURES + 1, 32), "n_features"), "65 features");
    REQUIRE(refused(ccdgpu_splits_check(x, n_rows, nf, 1), "max_bins"), "one bin");
    REQUIRE(refused(ccdgpu_splits_check(x, n_rows, nf, CCDGPU_TRAIN_MAX_EDGES + 2), "max_bins"), "65 bins");
    REQUIRE(refused(ccdgpu_splits_check(x, CCDGPU_TRAIN_MAX_ROWS, nf, 0), "max_bins"), "the counts come before the values");
    // values: the last element of the block, and the first
    x[n_rows * nf - 1] = nan;
    REQUIRE(refused(ccdgpu_splits_check(x, n_rows, nf, 32), "x[4][2] is not finite"), "NaN value");
    x[n_rows * nf - 1] = -inf;
    REQUIRE(refused(ccdgpu_splits_check(x, n_rows, nf, 32), "x[4][2] is not finite"), "infinite value");
    REQUIRE(ccdgpu_splits_check(x, n_rows - 1, nf, 32) == 0, "the rows before it");
    x[0] = inf;
    REQUIRE(refused(ccdgpu_splits_check(x, n_rows, nf, 32), "x[0][0] is not finite"), "the first of two");
    x[0] = 0.0;
    x[n_rows * nf - 1] = 1e300;
    REQUIRE(ccdgpu_splits_check(x, n_rows, nf, 32) == 0, "a large finite value");
    std::free(x);
    return 0;
}

int main() {
    if (checks()) return 1;
    std::printf("ok\n");
    return 0;
}
