// ccd_products.h -- launchers of ccd_products.hip (annual change and land-cover product rasters from
// segments), called by ccdgpu_products.cpp.  All pointers are device pointers; a launcher returns 0, or
// -1 when the launch was refused.
#ifndef CCD_PRODUCTS_H
#define CCD_PRODUCTS_H
#include <stdint.h>

#include "../../include/ccdgpu.h"

// What the products need of one row or segment, reduced once (ccd_product_records): 32 bytes.
typedef struct CcdProductRecord {
    int32_t sday, eday, bday;
    uint32_t flags;                // CCD_PREC_MODEL | CCD_PREC_BREAK | CCD_PREC_COVER | clamped curqa << 8
    float scmag;                   // the row's change magnitude (the rule's scmag, were it the break of a year)
    uint8_t label1, label2, conf1, conf2;  // lcpri, lcsec, lcpconf, lcsconf, were it the row of a date
    uint32_t pad[2];
} CcdProductRecord;
#define CCD_PREC_MODEL 1u
#define CCD_PREC_BREAK 2u
#define CCD_PREC_COVER 4u  // the cover products of the row are defined

#ifdef __cplusplus
extern "C" {
#endif
// most pixels one ccdk_products launch takes
int64_t ccdk_products_max_pixels(void);
// rec [n_rows] of table rows; rfrawp [n_rows][n_classes] row-aligned, or nullptr (no cover products)
int ccdk_product_records_rows(const ccdgpu_row *rows, int64_t n_rows, const float *rfrawp, const ccdgpu_product_params *params,
                              CcdProductRecord *rec, void *stream);
// the same of the n_seg segments of a chip of a run's CSR (magnitude and change_probability narrowed
// to float32 as the row packer does, every segment a model).  The rfrawp row of segment s, which pixel
// p holds (seg_off[p] <= s < seg_off[p + 1]), is row_off[p] + s - seg_off[p] (seg_off, row_off
// [n_pix + 1]: make_row_offsets); a segment whose row falls outside its pixel's rows or [0, n_rf_rows)
// has undefined cover products.
int ccdk_product_records_segments(const ccdgpu_segment *seg, int64_t n_seg, const float *rfrawp, int64_t n_rf_rows,
                                  const int64_t *seg_off, const int64_t *row_off, int64_t n_pix,
                                  const ccdgpu_product_params *params, CcdProductRecord *rec, void *stream);
// Pixel p (0 .. n_pix-1) has the records rec[off[p] - off_base .. off[p + 1] - off_base), all inside
// [0, n_rec) (a pixel whose range is not has no rows).  win [3][n_dates]: the dates, a and b of the
// rule.  out: device planes [n_dates][n_pix], nullptr for a product that is not wanted.
int ccdk_products(const CcdProductRecord *rec, int64_t n_rec, const int64_t *off, int64_t off_base, int64_t n_pix,
                  const int64_t *win, int64_t n_dates, const ccdgpu_product_params *params, const struct ccdgpu_products *out,
                  void *stream);
#ifdef __cplusplus
}
#endif
#endif
