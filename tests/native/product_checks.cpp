/* CPU check of the product request's validators and the year window
 * (lcmap-firebird_amd/csrc/ccdgpu_checks.cpp): a stand-alone program, built with
 * -fsanitize=address,undefined and run by tests/test_products.py.
 *  - ccdgpu_year_window over every day of the years around the century and leap boundaries, at 1 and
 *    at CCDGPU_PREDICT_MAX_DATE: a <= t < b, windows of 365 or 366 days that tile the calendar;
 *  - ccdgpu_products_check on tables, dates, rfrawp and label arrays given in heap blocks of exactly
 *    their size, so a read past them is a sanitizer error: the accepted edge cases and every rejection. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ccdgpu.h"

#define REQUIRE(cond, what)                                                                 \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::printf("%s:%d: %s (%s) -- %s\n", __FILE__, __LINE__, what, #cond, ccdgpu_last_error()); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

static bool refused(int rc, const char *needle) { return rc == CCDGPU_EINVAL && std::strstr(ccdgpu_last_error(), needle); }

static int year_windows() {
    int64_t a = 0, b = 0;
    REQUIRE(ccdgpu_year_window(1, &a, &b) == 0 && a == 1 && b == 366, "year 1");
    REQUIRE(ccdgpu_year_window(CCDGPU_PREDICT_MAX_DATE, &a, &b) == 0 && b == CCDGPU_PREDICT_MAX_DATE + 1 && b - a == 365, "year 9999");
    REQUIRE(refused(ccdgpu_year_window(0, &a, &b), "outside"), "t = 0");
    REQUIRE(refused(ccdgpu_year_window(CCDGPU_PREDICT_MAX_DATE + 1, &a, &b), "outside"), "t past the last day");
    REQUIRE(refused(ccdgpu_year_window(5, nullptr, &b), "NULL"), "NULL a");
    // 1 January 1890 .. 31 December 2110 (ordinals 689944 .. 770661): 1900 and 2100 are not leap years,
    // 2000 is; walk the days and require the windows to tile them
    int64_t pa = 0, pb = 0, years = 0, leaps = 0;
    for (int64_t t = 689944; t <= 770661; ++t) {
        REQUIRE(ccdgpu_year_window(t, &a, &b) == 0, "year window");
        REQUIRE(a <= t && t < b && (b - a == 365 || b - a == 366), "window holds its day");
        if (a != pa) {
            REQUIRE(pa == 0 || a == pb, "windows tile the calendar");
            REQUIRE(t == a, "a window starts on its first day");
            ++years;
            leaps += b - a == 366;
        }
        pa = a;
        pb = b;
    }
    REQUIRE(years == 221 && leaps == 53, "221 years with 53 leap years (not 1900, not 2100)");
    return 0;
}

static int checks() {
    // 3 pixels with 2, 0 and 1 rows; everything in heap blocks of exactly its size
    const int64_t n_pix = 3, n_rows = 3, n_dates = 2, nc = 4;
    int64_t *off = (int64_t *)std::malloc(sizeof(int64_t) * (n_pix + 1));
    ccdgpu_row *rows = (ccdgpu_row *)std::calloc(n_rows, sizeof(ccdgpu_row));
    int64_t *dates = (int64_t *)std::malloc(sizeof(int64_t) * n_dates);
    float *rf = (float *)std::calloc(n_rows * nc, sizeof(float));
    ccdgpu_product_params *p = (ccdgpu_product_params *)std::malloc(sizeof(ccdgpu_product_params));
    struct ccdgpu_products *o = (struct ccdgpu_products *)std::calloc(1, sizeof(struct ccdgpu_products));
    off[0] = 0, off[1] = 2, off[2] = 2, off[3] = 3;
    dates[0] = 727000, dates[1] = 1;
    ccdgpu_product_params_default(p);
    REQUIRE(p->bot == 723546 && p->mag_bands == 0x3E && p->cover == CCDGPU_COVER_EXTEND && p->n_classes == 0 &&
                p->labels[0] == 1 && p->labels[31] == 32,
            "default parameters");
    uint16_t dummy16 = 0;
    uint8_t dummy8 = 0;
    o->sctime = &dummy16;  // (pointers are only tested, never written)
    REQUIRE(ccdgpu_products_check(n_pix, off, n_rows, rows, nullptr, n_dates, dates, p, o) == 0, "change products alone");
    REQUIRE(ccdgpu_products_check(0, off, 0, nullptr, nullptr, 0, nullptr, p, o) == 0, "nothing at all");
    p->n_classes = (int32_t)nc;
    o->lcachg = &dummy16;
    REQUIRE(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o) == 0, "lcachg without lcpri");
    p->n_classes = 32;
    p->bot = CCDGPU_PREDICT_MAX_DATE;
    p->cover = CCDGPU_COVER_SPAN;
    o->lcachg = nullptr;
    REQUIRE(ccdgpu_products_check(n_pix, off, n_rows, rows, nullptr, n_dates, dates, p, o) == 0, "32 classes, bot at the last day");
    ccdgpu_product_params_default(p);
    p->n_classes = (int32_t)nc;
    // the prediction check's rejections of counts, offsets and dates
    REQUIRE(refused(ccdgpu_products_check(-1, off, n_rows, rows, rf, n_dates, dates, p, o), "n_pix"), "negative n_pix");
    REQUIRE(refused(ccdgpu_products_check(n_pix, nullptr, n_rows, rows, rf, n_dates, dates, p, o), "row_offsets is NULL"), "NULL offsets");
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, nullptr, rf, n_dates, dates, p, o), "rows is NULL"), "NULL rows");
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows + 1, rows, rf, n_dates, dates, p, o), "n_rows is"), "n_rows");
    off[1] = 3;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "decrease"), "decreasing offsets");
    off[1] = 2;
    off[0] = 1;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "row_offsets[0]"), "offsets start");
    off[0] = 0;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, nullptr, p, o), "dates is NULL"), "NULL dates");
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, -1, dates, p, o), "n_dates"), "negative n_dates");
    dates[1] = 0;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "dates[1]"), "date 0");
    dates[1] = CCDGPU_PREDICT_MAX_DATE + 1;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "dates[1]"), "date past the last");
    dates[1] = CCDGPU_PREDICT_MAX_DATE;
    REQUIRE(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o) == 0, "the last day is a date");
    // the product request's own
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, nullptr, o), "params is NULL"), "NULL params");
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, nullptr), "out is NULL"), "NULL out");
    p->bot = 0;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "bot"), "bot 0");
    p->bot = CCDGPU_PREDICT_MAX_DATE + 1;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "bot"), "bot past the last day");
    p->bot = 723546;
    p->mag_bands = 0x80;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "mag_bands"), "band bit 7");
    p->mag_bands = 0;
    REQUIRE(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o) == 0, "no magnitude band is a choice");
    p->mag_bands = 0x3E;
    p->n_classes = -1;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "n_classes"), "n_classes -1");
    p->n_classes = 33;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "n_classes"), "n_classes 33");
    p->n_classes = (int32_t)nc;
    p->labels[3] = 0;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "labels[3]"), "label 0");
    p->n_classes = 3;
    REQUIRE(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o) == 0, "a label of 0 past n_classes");
    p->n_classes = (int32_t)nc;
    p->labels[3] = 4;
    p->cover = 2;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "cover"), "unknown cover");
    p->cover = CCDGPU_COVER_EXTEND;
    o->lcsconf = &dummy8;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, nullptr, n_dates, dates, p, o), "rfrawp is NULL"), "cover without rfrawp");
    p->n_classes = 0;
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "n_classes is 0"), "cover without classes");
    std::memset(o, 0, sizeof(*o));
    REQUIRE(refused(ccdgpu_products_check(n_pix, off, n_rows, rows, rf, n_dates, dates, p, o), "no product"), "all ten NULL");
    std::free(off);
    std::free(rows);
    std::free(dates);
    std::free(rf);
    std::free(p);
    std::free(o);
    return 0;
}

int main() {
    if (year_windows() || checks()) return 1;
    std::printf("ok\n");
    return 0;
}
