// ccd_train.h -- random-forest training (include/ccdgpu.h states the rule): the rule's hash and
// row weight, written once for the host (feature subsets, ccdgpu_train.cpp) and the device (row
// weights, ccd_train.hip), and the launchers of ccd_train.hip.  All pointers of the launchers are
// device pointers; a launcher returns 0, or -1 when the launch was refused.
#ifndef CCD_TRAIN_H
#define CCD_TRAIN_H
#include <stdint.h>

#include "../../include/ccdgpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CCD_TRAIN_HD __host__ __device__ inline
#else
#define CCD_TRAIN_HD inline
#endif

#define CCD_TRAIN_GOLDEN 0x9E3779B97F4A7C15ull

CCD_TRAIN_HD uint64_t ccd_train_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
CCD_TRAIN_HD uint64_t ccd_train_fold(uint64_t z, uint64_t v) { return ccd_train_mix(z + CCD_TRAIN_GOLDEN + v); }
// H(seed, a, b, c) of the rule; ccd_train_hash_a is its (seed, a) prefix, shared by a tree's draws
CCD_TRAIN_HD uint64_t ccd_train_hash_a(uint64_t seed, uint64_t a) {
    return ccd_train_fold(ccd_train_mix(seed + CCD_TRAIN_GOLDEN), a);
}
CCD_TRAIN_HD uint64_t ccd_train_hash(uint64_t seed, uint64_t a, uint64_t b, uint64_t c) {
    return ccd_train_fold(ccd_train_fold(ccd_train_hash_a(seed, a), b), c);
}
// the Poisson(1) weight of the 32-bit draw u: the number of k with u >= CCDGPU_TRAIN_POISSON[k]
CCD_TRAIN_HD uint32_t ccd_train_poisson(uint32_t u) {
    const uint32_t P[CCDGPU_TRAIN_POISSON_N] = CCDGPU_TRAIN_POISSON;
    uint32_t w = 0;
    for (int k = 0; k < CCDGPU_TRAIN_POISSON_N; ++k) w += u >= P[k];
    return w;
}
// w(t, r) from tree_key = ccd_train_hash_a(seed, t)
CCD_TRAIN_HD uint32_t ccd_train_weight(uint64_t tree_key, uint64_t r, int bootstrap) {
    if (!bootstrap) return 1u;
    return ccd_train_poisson((uint32_t)(ccd_train_fold(ccd_train_fold(tree_key, r), 0) >> 32));
}

// The permutation rule's donor (a*r + b) mod n for a, b, r < n <= CCDGPU_TRAIN_MAX_ROWS, inv_n = 1.0 / n:
// p = a*r + b < n^2, so the quotient is below 2^27 + 1 and its estimate in double (three roundings of
// 2^-53 each) is off by far less than 1: once truncated it is the quotient or its neighbour, and one
// step either way gives the exact remainder without a 64-bit division.
CCD_TRAIN_HD uint64_t ccd_perm_donor(uint32_t a, uint32_t b, uint64_t r, uint64_t n, double inv_n) {
    const uint64_t p = (uint64_t)a * r + b;
    const uint64_t q = (uint64_t)((double)p * inv_n);
    const int64_t rem = (int64_t)(p - q * n);
    return (uint64_t)(rem < 0 ? rem + (int64_t)n : rem >= (int64_t)n ? rem - (int64_t)n : rem);
}

// bytes of LDS a histogram block may use for its private counters; a level whose largest tree needs
// more takes the global path
#define CCD_TRAIN_LDS_BYTES 49152
// rows one histogram block accumulates before it flushes its private counters
#define CCD_TRAIN_BLOCK_ROWS 4096

// what a level's kernels share
typedef struct CcdTrainLevel {
    const uint8_t *bins;        // [n_features][n_rows]
    const int32_t *labels;      // [n_rows]
    int32_t *slot;              // [n_group_trees][n_rows]: the row's node of this level, as an index
                                // into the level's node list; -1: not in the bag, or in a leaf
    const int32_t *tree_first;  // [n_group_trees + 1]: tree g's nodes are tree_first[g] .. tree_first[g + 1]
    const int32_t *subset;      // [n_nodes][m] features of each node, ascending
    uint32_t *hist;             // [n_nodes][m][n_bins][n_classes]
    const int32_t *n_edges;     // [n_features]
    int64_t n_rows;
    int32_t n_group_trees, n_nodes, m, n_bins, n_classes;
    int32_t first_tree;         // tree index of the group's first tree
    int32_t bootstrap;
    uint64_t seed;
} CcdTrainLevel;

#ifdef __cplusplus
extern "C" {
#endif
// bins [n_features][n_rows] of rows r0 .. r0 + n - 1, x [n][n_features] holding those rows; edges of
// feature f at edges[edge_off[f] .. edge_off[f + 1])
int ccdk_train_bin(const double *x, int64_t r0, int64_t n, int64_t n_rows, int32_t n_features, const double *edges,
                   const int32_t *edge_off, uint8_t *bins, void *stream);
// slot = 0-based root of the row's tree (tree g's root is node g of level 0) for rows in the bag, else -1
int ccdk_train_init(const CcdTrainLevel *lv, void *stream);
// (a) zero and fill the level's histograms; lds_bytes > 0: privatise them per block in that much LDS
// (the bytes of the counters of the tree with the most nodes, at most CCD_TRAIN_LDS_BYTES); 0: the
// global path
int ccdk_train_hist(const CcdTrainLevel *lv, int32_t lds_bytes, void *stream);
// (b) per node: split [n_nodes][2] = (feature, bin) of the chosen candidate or (-1, -1); counts
// [n_nodes][2][n_classes] = the node's class counts, then the chosen candidate's left counts
int ccdk_train_split(const CcdTrainLevel *lv, int32_t min_instances, double min_info_gain, int32_t *split, uint32_t *counts,
                     void *stream);
// (c) move every row to its child: child [n_nodes][2] = the left and right child's index in the next
// level's node list, -1 for a leaf
int ccdk_train_assign(const CcdTrainLevel *lv, const int32_t *split, const int32_t *child, void *stream);
#ifdef __cplusplus
}
#endif
#endif
