// ccd_predict.h -- launchers of ccd_predict.hip (prediction of band values from segment models),
// called by ccdgpu_predict.cpp.  All pointers are device pointers; a launcher returns 0, or -1 when the
// launch was refused.
#ifndef CCD_PREDICT_H
#define CCD_PREDICT_H
#include <stdint.h>

#include "../../include/ccdgpu.h"

// models a block of ccd_predict keeps in LDS at a time; a pixel with more is taken in pieces
#define CCD_PREDICT_CACHE_ROWS 16

#ifdef __cplusplus
extern "C" {
#endif
// basis [n_dates][8] doubles of dates [n_dates]: t, cos/sin of 1, 2, 3 cycles per year, 0
int ccdk_predict_basis(const int64_t *dates, int64_t n_dates, double avg_days_yr, double *basis, void *stream);
// most pixels one ccdk_predict_* launch takes
int64_t ccdk_predict_max_pixels(void);
// Pixel p (0 .. n_pix-1) has the models rows[off[p] - off_base .. off[p + 1] - off_base), all inside
// [0, n_models) (a pixel whose range is not gets the fill).  out: [7][n_pix][n_dates] of float
// (CCDGPU_PREDICT_F32) or int16 (CCDGPU_PREDICT_I16); seg_index [n_pix][n_dates] or nullptr.
int ccdk_predict_rows(const ccdgpu_row *rows, const int64_t *off, int64_t off_base, int64_t n_models, int64_t n_pix,
                      const int64_t *dates, const double *basis, int64_t n_dates, int32_t cover, int32_t dtype, void *out,
                      int32_t *seg_index, void *stream);
// the same over the segments of a run's CSR: every value narrowed to float32 as the row packer does
// (ccd_rows.hip), every segment a row with has_model 1
int ccdk_predict_segments(const ccdgpu_segment *seg, const int64_t *off, int64_t off_base, int64_t n_models, int64_t n_pix,
                          const int64_t *dates, const double *basis, int64_t n_dates, int32_t cover, int32_t dtype, void *out,
                          int32_t *seg_index, void *stream);
#ifdef __cplusplus
}
#endif
#endif
