/* CPU check of the permutation request's validator (lcmap-firebird_amd/csrc/ccdgpu_checks.cpp) and of
 * the donor arithmetic the kernel uses (csrc/ccd_train.h, ccd_perm_donor: a remainder without a 64-bit
 * division): a stand-alone program, built with -fsanitize=address,undefined and run by
 * tests/test_randomforest_permutation.py.  The labels sit in a heap block of exactly their size, which
 * the check scans; x and the outputs are arrays of one element (the check reads none of them). */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ccdgpu.h"
#include "../../lcmap-firebird_amd/csrc/ccd_train.h"

#define REQUIRE(cond, what)                                                                 \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::printf("%s:%d: %s (%s) -- %s\n", __FILE__, __LINE__, what, #cond, ccdgpu_last_error()); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

static bool refused(int rc, const char *needle) {
    const char *e = ccdgpu_last_error();
    return rc == CCDGPU_EINVAL && std::strncmp(e, "permutation: ", 13) == 0 && std::strstr(e, needle);
}

static int checks() {
    const int64_t top = CCDGPU_TRAIN_MAX_ROWS;
    const int64_t n = 5;
    double *x = (double *)std::malloc(sizeof(double));
    int32_t *y = (int32_t *)std::malloc(sizeof(int32_t) * n);
    int64_t *o = (int64_t *)std::malloc(sizeof(int64_t));
    ccdgpu_permutation_params *p = (ccdgpu_permutation_params *)std::malloc(sizeof(ccdgpu_permutation_params));
    p->seed = ~(uint64_t)0;
    p->perm_seed = ~(uint64_t)0;
    for (int64_t i = 0; i < n; ++i) y[i] = (int32_t)(i % 3);
    REQUIRE(ccdgpu_permutation_check(x, y, n, 2, 3, p, o, o, o, o) == 0, "a good request");
    REQUIRE(ccdgpu_permutation_check(nullptr, nullptr, 0, 2, 3, p, o, o, o, o) == 0, "no rows: x and labels may be NULL");
    REQUIRE(ccdgpu_permutation_check(x, y, n, CCDGPU_FOREST_MAX_FEATURES, CCDGPU_FOREST_MAX_CLASSES, p, o, o, o, o) == 0,
            "the largest feature and class counts");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, 3, nullptr, o, o, o, o), "params is NULL"), "NULL params");
    REQUIRE(refused(ccdgpu_permutation_check(nullptr, y, n, 2, 3, p, o, o, o, o), "x is NULL"), "NULL x");
    REQUIRE(refused(ccdgpu_permutation_check(x, nullptr, n, 2, 3, p, o, o, o, o), "labels is NULL"), "NULL labels");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, 3, p, nullptr, o, o, o), "oob_rows is NULL"), "NULL oob_rows");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, 3, p, o, nullptr, o, o), "correct is NULL"), "NULL correct");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, 3, p, o, o, nullptr, o), "lost is NULL"), "NULL lost");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, 3, p, o, o, o, nullptr), "gained is NULL"), "NULL gained");
    REQUIRE(refused(ccdgpu_permutation_check(nullptr, nullptr, 0, 2, 3, p, nullptr, o, o, o), "oob_rows is NULL"),
            "no rows still zero the outputs");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, -1, 2, 3, p, o, o, o, o), "n_rows"), "negative n_rows");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, top + 1, 2, 3, p, o, o, o, o), "n_rows"), "too many rows");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, INT64_MAX, 2, 3, p, o, o, o, o), "n_rows"), "n_rows at int64's end");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 0, 3, p, o, o, o, o), "n_features"), "no features");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, CCDGPU_FOREST_MAX_FEATURES + 1, 3, p, o, o, o, o), "n_features"),
            "too many features");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, 0, p, o, o, o, o), "n_classes"), "no classes");
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, CCDGPU_FOREST_MAX_CLASSES + 1, p, o, o, o, o), "n_classes"),
            "too many classes");
    y[n - 1] = 3;
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, 3, p, o, o, o, o), "labels[4] = 3"), "a label equal to n_classes");
    REQUIRE(ccdgpu_permutation_check(x, y, n - 1, 2, 3, p, o, o, o, o) == 0, "the bad label is past the rows");
    y[0] = -1;
    REQUIRE(refused(ccdgpu_permutation_check(x, y, n, 2, 3, p, o, o, o, o), "labels[0] = -1"), "a negative label, the first bad one");
    std::free(x);
    std::free(y);
    std::free(o);
    std::free(p);
    return 0;
}

/* ccd_perm_donor against the 64-bit remainder it stands for: small n in full, then large n (up to the
 * row limit, where a*r + b is just below 2^54) at the ends of every range and at hashed values */
static int donors() {
    for (uint64_t n = 1; n <= 40; ++n)
        for (uint64_t a = 0; a < n; ++a)
            for (uint64_t b = 0; b < n; ++b)
                for (uint64_t r = 0; r < n; ++r)
                    REQUIRE(ccd_perm_donor((uint32_t)a, (uint32_t)b, r, n, 1.0 / (double)n) == (a * r + b) % n, "small n");
    const uint64_t top = CCDGPU_TRAIN_MAX_ROWS;
    const uint64_t sizes[] = {top, top - 1, top - 2, (top >> 1) + 1, 1000003, (1u << 20) + 3, 99991, 4097};
    for (uint64_t n : sizes) {
        const double inv = 1.0 / (double)n;
        const uint64_t ends[] = {0, 1, 2, n / 2, n - 2, n - 1};
        for (uint64_t a : ends)
            for (uint64_t b : ends)
                for (uint64_t r : ends)
                    REQUIRE(ccd_perm_donor((uint32_t)a, (uint32_t)b, r, n, inv) == (a * r + b) % n, "the ends of the ranges");
        for (uint64_t i = 0; i < 200000; ++i) {
            const uint64_t k = ccd_train_hash(n, i, 1, 2), a = (k & 0xffffffffu) % n, b = (k >> 32) % n;
            const uint64_t r = ccd_train_hash(n, i, 3, 4) % n;
            REQUIRE(ccd_perm_donor((uint32_t)a, (uint32_t)b, r, n, inv) == (a * r + b) % n, "hashed values");
        }
        /* products next to a multiple of n, where a wrong quotient estimate would show */
        for (uint64_t a = n - 1; a > n - 300; --a) {
            const uint64_t r = n - 1, b = (n - (a * r) % n) % n;
            REQUIRE(ccd_perm_donor((uint32_t)a, (uint32_t)b, r, n, inv) == 0, "an exact multiple of n");
            if (b > 0) REQUIRE(ccd_perm_donor((uint32_t)a, (uint32_t)(b - 1), r, n, inv) == n - 1, "one below a multiple of n");
        }
    }
    return 0;
}

int main() {
    if (checks() || donors()) return 1;
    std::printf("ok\n");
    return 0;
}
