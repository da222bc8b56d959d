// ccd_splits.h -- the random forest's bin edges on the device (include/ccdgpu.h states the rule in
// its position form): the launchers of ccd_splits.hip, driven by ccdgpu_splits.cpp.  All pointers of
// the launchers are device pointers; a launcher returns 0, or -1 when the launch was refused.
//
// A group of G features is sorted at a time.  Its keys are feature-major uint64, [G][n_rows], in two
// buffers the radix passes go between; `plan` says per pass and column which buffer the pass reads
// (0 or 1) or that the column skips the pass (-1: all its keys share the digit), and `sorted_in` which
// buffer holds the column's sorted keys when the passes are done.  The other buffer of the column is
// then free and takes the column's boundary positions (int32, at most n_rows - 1 of them).
#ifndef CCD_SPLITS_H
#define CCD_SPLITS_H
#include <stdint.h>

#include "../../include/ccdgpu.h"

// keys one block of the sort and of the boundary kernels takes: 256 lanes of 16 keys each
#define CCD_SPLITS_TILE 4096
// 8 passes over 8-bit digits, least significant first
#define CCD_SPLITS_PASSES 8
#define CCD_SPLITS_DIGITS 256

typedef struct CcdSplitsGroup {
    uint64_t *keys[2];     // [G][n_rows] each
    int64_t n_rows;
    int32_t n_group;       // G
    int32_t n_tiles;       // ceil(n_rows / CCD_SPLITS_TILE)
    uint32_t *ghist;       // [G][CCD_SPLITS_PASSES][CCD_SPLITS_DIGITS]: the columns' digit counts of every pass
    uint32_t *counts;      // [G][CCD_SPLITS_DIGITS][n_tiles]: a pass's per-tile digit counts, then their offsets
    const int8_t *plan;    // [CCD_SPLITS_PASSES][G]
    const int8_t *sorted_in;  // [G]
    uint32_t *bcount;      // [G][n_tiles + 1]: boundaries per tile, then their offsets; [n_tiles]: the column's total
} CcdSplitsGroup;

#ifdef __cplusplus
extern "C" {
#endif
// keys[0] of rows r0 .. r0 + n - 1 for features f0 .. f0 + G - 1, x [n][n_features] holding those rows
int ccdk_splits_keys(const CcdSplitsGroup *g, const double *x, int64_t r0, int64_t n, int32_t n_features, int32_t f0,
                     void *stream);
// ghist of keys[0] (zeroed here first)
int ccdk_splits_ghist(const CcdSplitsGroup *g, void *stream);
// one radix pass of the columns whose plan is not -1: per-tile digit counts, their offsets, the scatter
int ccdk_splits_pass(const CcdSplitsGroup *g, int32_t pass, void *stream);
// boundaries of the sorted columns, laid down in order, and the walk of the rule: edges
// [G][CCDGPU_TRAIN_MAX_EDGES], n_edges [G]
int ccdk_splits_edges(const CcdSplitsGroup *g, int32_t max_bins, double *edges, int32_t *n_edges, void *stream);
#ifdef __cplusplus
}
#endif
#endif
