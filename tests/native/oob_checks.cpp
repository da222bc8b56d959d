/* CPU check of the out-of-bag request's validator (lcmap-firebird_amd/csrc/ccdgpu_checks.cpp): a
 * stand-alone program, built with -fsanitize=address,undefined and run by
 * tests/test_randomforest_oob.py.  ccdgpu_oob_check with the parameters in a heap block of exactly
 * their size and arrays of one element (the check reads none of them): the accepted edge cases and
 * every rejection. */
#include <cstdio>
#include <cstdlib>
#include <cstring>

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
    const int64_t top = CCDGPU_TRAIN_MAX_ROWS;
    double *x = (double *)std::malloc(sizeof(double));
    float *raw = (float *)std::malloc(sizeof(float));
    int32_t *n = (int32_t *)std::malloc(sizeof(int32_t));
    ccdgpu_oob_params *p = (ccdgpu_oob_params *)std::malloc(sizeof(ccdgpu_oob_params));
    p->seed = ~(uint64_t)0;
    p->first_row = 0;
    REQUIRE(ccdgpu_oob_check(x, 1, p, raw, n) == 0, "a good request");
    REQUIRE(ccdgpu_oob_check(x, top, p, raw, n) == 0, "2^27 rows from row 0 (x is not scanned)");
    REQUIRE(ccdgpu_oob_check(nullptr, 0, p, nullptr, nullptr) == 0, "no rows: the arrays may be NULL");
    p->first_row = top - 1;
    REQUIRE(ccdgpu_oob_check(x, 1, p, raw, n) == 0, "the last hash index");
    p->first_row = top;
    REQUIRE(ccdgpu_oob_check(nullptr, 0, p, nullptr, nullptr) == 0, "no rows at the end");
    REQUIRE(refused(ccdgpu_oob_check(x, 1, p, raw, n), "first_row"), "one row past the last hash index");
    p->first_row = -1;
    REQUIRE(refused(ccdgpu_oob_check(x, 1, p, raw, n), "first_row"), "negative first_row");
    p->first_row = INT64_MAX;
    REQUIRE(refused(ccdgpu_oob_check(x, 1, p, raw, n), "first_row"), "first_row + n_rows past int64");
    p->first_row = 0;
    REQUIRE(refused(ccdgpu_oob_check(x, -1, p, raw, n), "n_rows"), "negative n_rows");
    REQUIRE(refused(ccdgpu_oob_check(x, top + 1, p, raw, n), "n_rows"), "too many rows");
    REQUIRE(refused(ccdgpu_oob_check(x, INT64_MAX, p, raw, n), "n_rows"), "n_rows at int64's end");
    REQUIRE(refused(ccdgpu_oob_check(x, 1, nullptr, raw, n), "params is NULL"), "NULL params");
    REQUIRE(refused(ccdgpu_oob_check(nullptr, 1, p, raw, n), "x is NULL"), "NULL x");
    REQUIRE(refused(ccdgpu_oob_check(x, 1, p, nullptr, n), "oob_raw is NULL"), "NULL oob_raw");
    REQUIRE(refused(ccdgpu_oob_check(x, 1, p, raw, nullptr), "n_oob is NULL"), "NULL n_oob");
    std::free(x);
    std::free(raw);
    std::free(n);
    std::free(p);
    return 0;
}

int main() {
    if (checks()) return 1;
    std::printf("ok\n");
    return 0;
}
