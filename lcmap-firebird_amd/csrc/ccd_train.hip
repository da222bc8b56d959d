// ccd_train.hip -- random-forest training on the device (include/ccdgpu.h states the rule; the host
// loop over tree groups and levels is ccdgpu_train.cpp).
//
// A call bins its rows once (ccd_train_bin: a feature-major uint8 matrix).  Then, per level of a group
// of trees, three bounded launches:
//   (a) ccd_train_hist_*   weighted class histograms per (node of the level, subset feature, bin,
//                          class), uint32.  A block takes one tree and CCD_TRAIN_BLOCK_ROWS rows; while
//                          the tree's nodes of the level fit CCD_TRAIN_LDS_BYTES it counts into LDS and
//                          flushes the non-zero counters with one global add each, otherwise
//                          (ccd_train_hist_global) every row adds straight to global memory.  All adds
//                          are integer atomics whose return value is unused, so the counts do not
//                          depend on arrival order.
//   (b) ccd_train_split    one wave per node, one lane per bin: per subset feature a wave prefix sum
//                          over the bins gives every candidate's left counts; scores in double from
//                          int64 sums as the rule states them; argmax with the rule's tie order.
//   (c) ccd_train_assign   every row moves to its child's place in the next level's node list.
// Nothing is accumulated in floating point across lanes or blocks, and no block waits for another.
#include <hip/hip_runtime.h>

#include "ccd_train.h"

namespace {

constexpr int T = 256;

__global__ __launch_bounds__(T) void ccd_train_bin(const double *__restrict__ x, int64_t r0, int64_t n, int64_t n_rows,
                                                   int32_t nf, const double *__restrict__ edges,
                                                   const int32_t *__restrict__ edge_off, uint8_t *__restrict__ bins) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    if (i >= n * nf) return;
    const int64_t r = i / nf;
    const int32_t f = (int32_t)(i - r * nf);
    const double v = x[i];
    // the number of edges below v: the first edge that is >= v (edges ascend)
    int32_t lo = edge_off[f], hi = edge_off[f + 1];
    const int32_t base = lo;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (edges[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    bins[(size_t)f * (size_t)n_rows + (size_t)(r0 + r)] = (uint8_t)(lo - base);
}

__global__ __launch_bounds__(T) void ccd_train_init(CcdTrainLevel lv) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    const int32_t g = blockIdx.y;
    if (r >= lv.n_rows) return;
    const uint64_t key = ccd_train_hash_a(lv.seed, (uint64_t)(lv.first_tree + g));
    lv.slot[(size_t)g * (size_t)lv.n_rows + (size_t)r] = ccd_train_weight(key, (uint64_t)r, lv.bootstrap) ? g : -1;
}

// the counters a row adds to: to h + (its node's index - first) * per, one per subset feature
__device__ __forceinline__ void count_row(const CcdTrainLevel &lv, uint32_t *h, int32_t s, int32_t first, int64_t r, uint32_t w) {
    const int32_t k = lv.labels[r];
    if ((unsigned)k >= (unsigned)lv.n_classes) return;
    const size_t per_feature = (size_t)lv.n_bins * lv.n_classes;
    uint32_t *hn = h + (size_t)(s - first) * lv.m * per_feature;
    for (int32_t j = 0; j < lv.m; ++j) {
        const int32_t f = lv.subset[(size_t)s * lv.m + j];
        const int32_t b = lv.bins[(size_t)f * (size_t)lv.n_rows + (size_t)r];
        if (b < lv.n_bins) (void)atomicAdd(hn + j * per_feature + (size_t)b * lv.n_classes + k, w);
    }
}

__global__ __launch_bounds__(T) void ccd_train_hist_lds(CcdTrainLevel lv) {
    extern __shared__ uint32_t lds_hist[];
    const int32_t g = blockIdx.y;
    const int32_t first = lv.tree_first[g], nn = lv.tree_first[g + 1] - first;
    if (nn <= 0) return;  // (the whole block: no barrier is skipped by part of it)
    const int32_t per = lv.m * lv.n_bins * lv.n_classes, total = nn * per;
    for (int32_t i = threadIdx.x; i < total; i += T) lds_hist[i] = 0u;
    __syncthreads();
    const int64_t r_lo = (int64_t)blockIdx.x * CCD_TRAIN_BLOCK_ROWS;
    const int64_t r_hi = r_lo + CCD_TRAIN_BLOCK_ROWS < lv.n_rows ? r_lo + CCD_TRAIN_BLOCK_ROWS : lv.n_rows;
    const uint64_t key = ccd_train_hash_a(lv.seed, (uint64_t)(lv.first_tree + g));
    const int32_t *slot = lv.slot + (size_t)g * (size_t)lv.n_rows;
    for (int64_t r = r_lo + threadIdx.x; r < r_hi; r += T) {
        const int32_t s = slot[r];
        if (s < first || s >= first + nn) continue;
        const uint32_t w = ccd_train_weight(key, (uint64_t)r, lv.bootstrap);
        if (w) count_row(lv, lds_hist, s, first, r, w);
    }
    __syncthreads();
    uint32_t *out = lv.hist + (size_t)first * per;
    for (int32_t i = threadIdx.x; i < total; i += T) {
        const uint32_t v = lds_hist[i];
        if (v) (void)atomicAdd(out + i, v);
    }
}

__global__ __launch_bounds__(T) void ccd_train_hist_global(CcdTrainLevel lv) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    const int32_t g = blockIdx.y;
    if (r >= lv.n_rows) return;
    const int32_t s = lv.slot[(size_t)g * (size_t)lv.n_rows + (size_t)r];
    if (s < 0 || s >= lv.n_nodes) return;
    const uint32_t w = ccd_train_weight(ccd_train_hash_a(lv.seed, (uint64_t)(lv.first_tree + g)), (uint64_t)r, lv.bootstrap);
    if (w) count_row(lv, lv.hist, s, 0, r, w);
}

// is candidate (score o, feature place oj, bin ob) ahead of (score, j, b)?  A place < 0 is no candidate.
__device__ __forceinline__ bool ahead(double os, int32_t oj, int32_t ob, double score, int32_t j, int32_t b) {
    if (oj < 0) return false;
    if (j < 0) return true;
    if (os != score) return os > score;
    return oj != j ? oj < j : ob < b;
}

__global__ __launch_bounds__(64) void ccd_train_split(CcdTrainLevel lv, int32_t min_instances, double min_info_gain,
                                                      int32_t *__restrict__ split, uint32_t *__restrict__ counts) {
    __shared__ uint32_t tot[CCDGPU_FOREST_MAX_CLASSES];
    const int32_t s = blockIdx.x, lane = threadIdx.x;
    const int32_t C = lv.n_classes, nb = lv.n_bins, m = lv.m;
    const uint32_t *h = lv.hist + (size_t)s * m * nb * C;
    if (lane < C) {  // the node's class counts: every row is in one bin of its first subset feature
        uint32_t t = 0;
        for (int32_t b = 0; b < nb; ++b) t += h[(size_t)b * C + lane];
        tot[lane] = t;
    }
    __syncthreads();
    int64_t n = 0, q = 0;
    for (int32_t k = 0; k < C; ++k) {
        n += (int64_t)tot[k];
        q += (int64_t)tot[k] * (int64_t)tot[k];
    }
    double best = 0.0;
    int32_t best_j = -1;
    if (n > 0) {
        const double parent = (double)q / (double)n;
        for (int32_t j = 0; j < m; ++j) {
            const int32_t ne = lv.n_edges[lv.subset[(size_t)s * m + j]];
            int64_t nL = 0, qL = 0, qR = 0;
            for (int32_t k = 0; k < C; ++k) {
                uint32_t c = lane < nb ? h[((size_t)j * nb + lane) * C + k] : 0u;
                for (int d = 1; d < 64; d <<= 1) {  // inclusive prefix sum over the bins (lanes)
                    const uint32_t up = __shfl_up(c, d, 64);
                    if (lane >= d) c += up;
                }
                const int64_t cl = (int64_t)c, cr = (int64_t)tot[k] - cl;
                nL += cl;
                qL += cl * cl;
                qR += cr * cr;
            }
            const int64_t nR = n - nL;
            if (lane < ne && nL >= min_instances && nR >= min_instances) {
                const double score = (double)qL / (double)nL + (double)qR / (double)nR;
                const double gain = (score - parent) / (double)n;
                if (gain >= min_info_gain && (best_j < 0 || score > best)) {
                    best = score;
                    best_j = j;
                }
            }
        }
    }
    int32_t best_b = lane;
    for (int d = 32; d >= 1; d >>= 1) {
        const double os = __shfl_xor(best, d, 64);
        const int32_t oj = __shfl_xor(best_j, d, 64), ob = __shfl_xor(best_b, d, 64);
        if (ahead(os, oj, ob, best, best_j, best_b)) {
            best = os;
            best_j = oj;
            best_b = ob;
        }
    }
    if (lane == 0) {
        split[2 * (size_t)s] = best_j < 0 ? -1 : lv.subset[(size_t)s * m + best_j];
        split[2 * (size_t)s + 1] = best_j < 0 ? -1 : best_b;
    }
    if (lane < C) {
        uint32_t left = 0;
        if (best_j >= 0)
            for (int32_t b = 0; b <= best_b; ++b) left += h[((size_t)best_j * nb + b) * C + lane];
        counts[(size_t)s * 2 * C + lane] = tot[lane];
        counts[(size_t)s * 2 * C + C + lane] = left;
    }
}

__global__ __launch_bounds__(T) void ccd_train_assign(CcdTrainLevel lv, const int32_t *__restrict__ split,
                                                      const int32_t *__restrict__ child) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    const int32_t g = blockIdx.y;
    if (r >= lv.n_rows) return;
    int32_t *slot = lv.slot + (size_t)g * (size_t)lv.n_rows + (size_t)r;
    const int32_t s = *slot;
    if (s < 0) return;
    int32_t next = -1;
    if (s < lv.n_nodes && split[2 * (size_t)s] >= 0) {
        const int32_t b = lv.bins[(size_t)split[2 * (size_t)s] * (size_t)lv.n_rows + (size_t)r];
        next = child[2 * (size_t)s + (b <= split[2 * (size_t)s + 1] ? 0 : 1)];
    }
    *slot = next;
}

bool row_grid(const CcdTrainLevel *lv, dim3 *grid, int64_t rows_per_block) {
    const int64_t bx = (lv->n_rows + rows_per_block - 1) / rows_per_block;
    if (lv->n_rows <= 0 || bx > 0x7fffffff || lv->n_group_trees <= 0 || lv->n_group_trees > 65535) return false;
    *grid = dim3((unsigned)bx, (unsigned)lv->n_group_trees);
    return true;
}

}  // namespace

extern "C" int ccdk_train_bin(const double *x, int64_t r0, int64_t n, int64_t n_rows, int32_t n_features, const double *edges,
                              const int32_t *edge_off, uint8_t *bins, void *stream) {
    if (n <= 0) return 0;
    if (r0 < 0 || r0 + n > n_rows || n_features <= 0) return -1;
    const int64_t blocks = (n * n_features + T - 1) / T;
    if (blocks > 0x7fffffff) return -1;
    hipLaunchKernelGGL(ccd_train_bin, dim3((unsigned)blocks), dim3(T), 0, (hipStream_t)stream, x, r0, n, n_rows, n_features, edges,
                       edge_off, bins);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int ccdk_train_init(const CcdTrainLevel *lv, void *stream) {
    dim3 grid;
    if (!row_grid(lv, &grid, T)) return -1;
    hipLaunchKernelGGL(ccd_train_init, grid, dim3(T), 0, (hipStream_t)stream, *lv);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int ccdk_train_hist(const CcdTrainLevel *lv, int32_t lds_bytes, void *stream) {
    dim3 grid;
    if (lv->n_nodes <= 0 || lds_bytes < 0 || lds_bytes > CCD_TRAIN_LDS_BYTES) return -1;
    const size_t bytes = sizeof(uint32_t) * (size_t)lv->n_nodes * lv->m * lv->n_bins * lv->n_classes;
    if (hipMemsetAsync(lv->hist, 0, bytes, (hipStream_t)stream) != hipSuccess) return -1;
    if (lds_bytes > 0) {
        if (!row_grid(lv, &grid, CCD_TRAIN_BLOCK_ROWS)) return -1;
        hipLaunchKernelGGL(ccd_train_hist_lds, grid, dim3(T), (size_t)lds_bytes, (hipStream_t)stream, *lv);
    } else {
        if (!row_grid(lv, &grid, T)) return -1;
        hipLaunchKernelGGL(ccd_train_hist_global, grid, dim3(T), 0, (hipStream_t)stream, *lv);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int ccdk_train_split(const CcdTrainLevel *lv, int32_t min_instances, double min_info_gain, int32_t *split,
                                uint32_t *counts, void *stream) {
    if (lv->n_nodes <= 0 || lv->n_bins > 64 || lv->n_classes > CCDGPU_FOREST_MAX_CLASSES) return -1;
    hipLaunchKernelGGL(ccd_train_split, dim3((unsigned)lv->n_nodes), dim3(64), 0, (hipStream_t)stream, *lv, min_instances,
                       min_info_gain, split, counts);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int ccdk_train_assign(const CcdTrainLevel *lv, const int32_t *split, const int32_t *child, void *stream) {
    dim3 grid;
    if (!row_grid(lv, &grid, T)) return -1;
    hipLaunchKernelGGL(ccd_train_assign, grid, dim3(T), 0, (hipStream_t)stream, *lv, split, child);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
