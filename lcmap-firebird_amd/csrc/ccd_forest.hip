// ccd_forest.hip -- MI355X (gfx950) random-forest inference over segment rows: the `rfrawp`
// column of the segment table.
//
// Reference: ccdc/randomforest.py:25-87 classifies the feature vectors of ccdc/features.py with
// Spark ML's RandomForestClassificationModel (500 trees) and keeps its rawPrediction -- per row,
// the sum over the trees, in tree order, of the reached leaf's normalised class distribution --
// as array<float>.  include/ccdgpu.h states the walk; this kernel reproduces it exactly.
//
// One lane per row walks every tree in order and keeps n_classes double accumulators, so the
// additions of a row happen in tree order whatever the launch shape.  A block's feature vectors
// sit in LDS as [feature][row] (the feature index of a node is data, so registers cannot hold
// them; lanes of a wave that test the same feature read consecutive doubles).  The forest streams
// through the rest of the block's LDS in chunks of whole trees (ccd_device.h, CcdForestDev): the
// block copies a chunk, every lane walks its trees out of LDS, the next chunk follows.  A tree
// larger than a chunk is walked from global memory (L2) by the same code.  A node is 16 bytes
// (threshold, feature, left child; the right child is the next node), read as one b128; the
// leaves' class vectors follow the nodes of their tree, so a chunk carries them too.
//
// ccd_forest_oob is the same walk for the out-of-bag estimate: a row takes only the trees whose bag
// it is not in, by the training rule's hash (ccd_train.h).  ccd_forest_permutation counts, per tree
// over the rows out of its bag, the right votes and those lost or gained under a shuffled feature.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/ccdgpu.h"
#include "ccd_device.h"
#include "ccd_train.h"

namespace {

constexpr int W = 64;
constexpr int LDS_BYTES = 160 * 1024;   // per CU, and the most one block may ask for
constexpr int MIN_CHUNK = 16 * 1024;    // least chunk room a launch shape must leave
constexpr int GATHER_F = 33;            // ccdc.features.columns()

// bytes of a block's feature vectors: [n_features][threads + 1] doubles (the odd row stride keeps
// the transposing stores of the load off a single bank), rounded to the chunk's 16-byte alignment
__host__ __device__ constexpr int feat_bytes(int n_features, int threads) {
    return (n_features * (threads + 1) * 8 + 15) & ~15;
}

// A block's rows, as every walk sees them: the lane's row and its column of the LDS feature vectors,
// and the chunk room behind them.
struct BlockRows {
    const double *xs_lane;  // feature c of the lane's row is xs_lane[c * (T + 1)]
    unsigned char *chunk;
    int64_t row;
    int tid, nrow;  // lanes tid < nrow have a row
};

// The block frame of the three walks: splits the block's LDS, loads its rows -- row-major in global
// memory (coalesced) -- transposed into it, and places the lane.  False for a block past n_rows.
// The rows are in place for every lane only after for_each_chunk's first barrier.
template <int T>
__device__ __forceinline__ bool block_rows(const CcdForestDev &f, const double *x, int64_t n_rows, BlockRows &b) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int XS = T + 1;
    const int nf = f.n_features;
    double *xs = reinterpret_cast<double *>(smem);
    b.chunk = smem + feat_bytes(nf, T);
    b.tid = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * T;
    if (row0 >= n_rows) return false;
    b.nrow = n_rows - row0 < T ? (int)(n_rows - row0) : T;
    const double *xb = x + row0 * nf;
    for (int i = b.tid; i < b.nrow * nf; i += T) {
        const int r = i / nf, c = i - r * nf;
        xs[c * XS + r] = xb[i];
    }
    b.row = row0 + b.tid;
    b.xs_lane = xs + b.tid;
    return true;
}

// The chunk loop of the three walks: the block copies a chunk of whole trees into LDS and hands
// its trees [t0, t1) to `trees`; a tree larger than a chunk is handed over in global memory.  Tree
// t's blob is at src + (f.tree_off[t] - first).  Every lane of the block calls this and `trees`
// runs for every lane (the barriers; the permutation kernel's ballots), so a caller tests its
// lane's liveness inside `trees`.
template <int T, class Trees>
__device__ __forceinline__ void for_each_chunk(const CcdForestDev &f, const BlockRows &b, Trees &&trees) {
    for (int c = 0; c < f.n_chunks; ++c) {
        const int t0 = f.chunk_first[c], t1 = f.chunk_first[c + 1];
        const int64_t base = f.tree_off[t0];
        const int64_t bytes = f.tree_off[t1] - base;
        if (bytes <= (int64_t)f.chunk_cap) {
            __syncthreads();  // the feature vectors are in place / the previous chunk is done with
            const uint4 *src = reinterpret_cast<const uint4 *>(f.pool + base);
            uint4 *dst = reinterpret_cast<uint4 *>(b.chunk);
            for (int i = b.tid; i < (int)(bytes >> 4); i += T) dst[i] = src[i];
            __syncthreads();
            trees(t0, t1, static_cast<const unsigned char *>(b.chunk), base);
        } else {
            __syncthreads();  // (the feature vectors, when this is the first chunk)
            trees(t0, t1, f.pool, (int64_t)0);
        }
    }
}

constexpr uint32_t POISSON[CCDGPU_TRAIN_POISSON_N] = CCDGPU_TRAIN_POISSON;
static_assert(POISSON[0] == CCDGPU_OOB_CUT, "CCDGPU_OOB_CUT is the first entry of CCDGPU_TRAIN_POISSON");

// Row r (its hash index) is out of tree t's bag: the draw u = H(seed, t, r, 0) >> 32 is below P[0],
// i.e. w(t, r) == 0.  key = tree_key[t] = ccd_train_hash_a(seed, t), the same for every lane (a
// scalar load per tree); the lane folds r and 0 into it.
__device__ __forceinline__ bool out_of_bag(uint64_t key, uint64_t r) {
    return (uint32_t)(ccd_train_fold(ccd_train_fold(key, r), 0) >> 32) < CCDGPU_OOB_CUT;
}

static_assert(CCDGPU_FOREST_MAX_FEATURES <= 64, "the features of a path are one bit each of a uint64");
static_assert(CCDGPU_FOREST_MAX_CLASSES <= W, "lane k of a wave sums the wave's counts of class k");

// One tree's descent for one row: at most max_depth branches (the checked forest's depth; a leaf
// is always reached within it), to the node reached.  SUB (the votes of the permutation counts):
// feature sub_f (-1: none) is read as sub_v and every tested feature's bit is set in `path`.
template <bool SUB>
__device__ __forceinline__ CcdForestNode descend(const unsigned char *blob, const double *xs_lane, int xs_stride, int max_depth,
                                                 int sub_f, double sub_v, uint64_t &path) {
    const CcdForestNode *nodes = reinterpret_cast<const CcdForestNode *>(blob);
    CcdForestNode nd = nodes[0];
    for (int d = 0; d < max_depth && nd.feature >= 0; ++d) {
        if (SUB) path |= 1ull << nd.feature;
        const double v = SUB && nd.feature == sub_f ? sub_v : xs_lane[nd.feature * xs_stride];
        nd = nodes[nd.left + (v <= nd.threshold ? 0 : 1)];  // NaN compares false: right
    }
    return nd;
}

// One tree for one row: the leaf's class vector added to the accumulators.
template <int NC>
__device__ __forceinline__ void walk(const unsigned char *blob, const double *xs_lane, int xs_stride, int max_depth, int nc,
                                     double (&acc)[NC]) {
    uint64_t unused = 0;
    const CcdForestNode nd = descend<false>(blob, xs_lane, xs_stride, max_depth, -1, 0.0, unused);
    if (nd.feature >= 0) return;  // (not reached for a checked forest)
    const double *val = reinterpret_cast<const double *>(blob) + nd.left;
#pragma unroll
    for (int k = 0; k < NC; ++k)
        if (k < nc) acc[k] += val[k];
}

// One tree for one row, for its vote: at the leaf the lowest class with the largest value.
__device__ __forceinline__ int vote(const unsigned char *blob, const double *xs_lane, int xs_stride, int max_depth, int nc,
                                    int sub_f, double sub_v, uint64_t &path) {
    const CcdForestNode nd = descend<true>(blob, xs_lane, xs_stride, max_depth, sub_f, sub_v, path);
    if (nd.feature >= 0) return -1;  // (not reached for a checked forest)
    const double *val = reinterpret_cast<const double *>(blob) + nd.left;
    int best = 0;
    double top = val[0];
    for (int k = 1; k < nc; ++k) {
        const double v = val[k];
        if (v > top) {
            top = v;
            best = k;
        }
    }
    return best;
}

// The classification: every live row takes every tree; a skipped row's prediction is NaN.
template <int NC, int T>
__global__ __launch_bounds__(T) void ccd_forest_classify(CcdForestDev f, const double *__restrict__ x,
                                                         const unsigned char *__restrict__ skip, int64_t n_rows,
                                                         float *__restrict__ out) {
    BlockRows b;
    if (!block_rows<T>(f, x, n_rows, b)) return;
    const int nc = f.n_classes;
    const bool live = b.tid < b.nrow && !(skip && skip[b.row]);
    double acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.0;
    for_each_chunk<T>(f, b, [&](int t0, int t1, const unsigned char *src, int64_t first) {
        if (live)
            for (int t = t0; t < t1; ++t) walk<NC>(src + (f.tree_off[t] - first), b.xs_lane, T + 1, f.max_depth, nc, acc);
    });
    if (b.tid < b.nrow) {
        float *o = out + b.row * nc;
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if (k < nc) o[k] = live ? __double2float_rn(acc[k]) : __uint_as_float(0x7fc00000u);
    }
}

// The out-of-bag walk (include/ccdgpu.h states the rule): ccd_forest_classify's layout -- one lane
// per row, feature vectors transposed in LDS, the trees streamed through LDS in chunks -- with the
// rule's membership test in front of every tree: the lane walks the tree only when out_of_bag.  The
// count of trees that scored the row stays in a register.  Rows past n_rows neither read nor write.
template <int NC, int T>
__global__ __launch_bounds__(T) void ccd_forest_oob(CcdForestDev f, const double *__restrict__ x,
                                                    const uint64_t *__restrict__ tree_key, uint64_t first_row, int64_t n_rows,
                                                    float *__restrict__ out, int32_t *__restrict__ n_oob) {
    BlockRows b;
    if (!block_rows<T>(f, x, n_rows, b)) return;
    const int nc = f.n_classes;
    const bool live = b.tid < b.nrow;
    const uint64_t r = first_row + (uint64_t)b.row;
    double acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.0;
    int32_t scored = 0;
    for_each_chunk<T>(f, b, [&](int t0, int t1, const unsigned char *src, int64_t first) {
        for (int t = t0; t < t1; ++t)
            if (live && out_of_bag(tree_key[t], r)) {
                walk<NC>(src + (f.tree_off[t] - first), b.xs_lane, T + 1, f.max_depth, nc, acc);
                ++scored;
            }
    });
    if (live) {
        float *o = out + b.row * nc;
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if (k < nc) o[k] = __double2float_rn(acc[k]);
        n_oob[b.row] = scored;
    }
}

// The out-of-bag permutation counts (include/ccdgpu.h states the rule): ccd_forest_oob's layout and
// membership test; a row out of a tree's bag takes the tree's vote, which also collects the features
// its path tests, and then one re-walk per such feature with the donor row's value (an 8-byte gather
// from x, which is whole in global memory) in its place -- a feature off the path cannot change the
// vote.  perm_ab [n_trees][n_features] = the (a, b) of each column's permutation, from the host.
// Counts: oob_rows and correct get an add from every row out of the bag, so a wave sums them first --
// lane k holds the wave's lanes of label k, two ballots per tree give it the wave's counts of class k
// -- and adds the non-zero sums, one per class; lost and gained are sparse (an add only where the
// vote's correctness changed, spread over n_features * n_classes counters per tree: too few per block
// and counter for an LDS copy to merge them) and go straight to global memory.  The block's feature
// vectors and the chunk fill the LDS at 33 features, so no counter lives there.  Rows past n_rows
// neither read, write nor count.
template <int T>
__global__ __launch_bounds__(T) void ccd_forest_permutation(CcdForestDev f, const double *__restrict__ x,
                                                            const int32_t *__restrict__ labels,
                                                            const uint64_t *__restrict__ tree_key,
                                                            const uint2 *__restrict__ perm_ab, int64_t n_rows,
                                                            uint32_t *__restrict__ oob_rows, uint32_t *__restrict__ correct,
                                                            uint32_t *__restrict__ lost, uint32_t *__restrict__ gained) {
    BlockRows b;
    if (!block_rows<T>(f, x, n_rows, b)) return;
    const int nf = f.n_features, nc = f.n_classes, lane = b.tid % W;
    const bool live = b.tid < b.nrow;
    const uint64_t r = (uint64_t)b.row, n = (uint64_t)n_rows;
    const int y = live ? labels[b.row] : 0;
    const double inv_n = 1.0 / (double)n_rows;
    uint64_t of_class = 0;  // in lane k: the wave's live lanes of label k
    for (int k = 0; k < nc; ++k) {
        const uint64_t m = __ballot(live && y == k);
        if (lane == k) of_class = m;
    }
    // every lane of the wave runs this (the ballots); `live` and `out` are tested inside
    auto one_tree = [&](int t, const unsigned char *blob) {
        const bool out = live && out_of_bag(tree_key[t], r);
        bool base = false;
        if (out) {
            uint64_t path = 0, unused = 0;
            base = vote(blob, b.xs_lane, T + 1, f.max_depth, nc, -1, 0.0, path) == y;
            const uint2 *ab = perm_ab + (int64_t)t * nf;
            while (path) {
                const int pf = __ffsll((unsigned long long)path) - 1;
                path &= path - 1;
                const uint2 p = ab[pf];
                const double v = x[ccd_perm_donor(p.x, p.y, r, n, inv_n) * nf + pf];
                const bool perm = vote(blob, b.xs_lane, T + 1, f.max_depth, nc, pf, v, unused) == y;
                if (perm != base) atomicAdd((base ? lost : gained) + ((int64_t)t * nf + pf) * nc + y, 1u);
            }
        }
        const uint64_t outs = __ballot(out), hits = __ballot(base);
        if (lane < nc) {
            const uint32_t n_out = (uint32_t)__popcll(outs & of_class), n_hit = (uint32_t)__popcll(hits & of_class);
            if (n_out) atomicAdd(oob_rows + (int64_t)t * nc + lane, n_out);
            if (n_hit) atomicAdd(correct + (int64_t)t * nc + lane, n_hit);
        }
    };
    for_each_chunk<T>(f, b, [&](int t0, int t1, const unsigned char *src, int64_t first) {
        for (int t = t0; t < t1; ++t) one_tree(t, src + (f.tree_off[t] - first));
    });
}

// The feature matrix of a run's rows, one wave per pixel, lanes over the elements of its rows:
// the float32 value the row packer stores (ccd_rows.hip) widened to double, then the pixel's aux
// values.  n_seg / n_rows bound every read and write.
__global__ __launch_bounds__(256) void ccd_forest_gather(const ccdgpu_segment *__restrict__ seg, const int64_t *__restrict__ seg_off,
                                                         const int64_t *__restrict__ row_off, const double *__restrict__ aux,
                                                         int64_t n_pix, int64_t n_seg, int64_t n_rows, double *__restrict__ x,
                                                         unsigned char *__restrict__ skip) {
    const int l = threadIdx.x % W;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x / W);
    for (int64_t p = (int64_t)blockIdx.x * (blockDim.x / W) + threadIdx.x / W; p < n_pix; p += nw) {
        const int64_t s0 = seg_off[p], ns = seg_off[p + 1] - s0, r0 = row_off[p];
        const int64_t nr = ns > 0 ? ns : 1;
        if (s0 < 0 || ns < 0 || s0 + ns > n_seg || r0 < 0 || r0 + nr > n_rows) continue;
        const double *ax = aux + p * 5;
        for (int64_t e = l; e < nr * GATHER_F; e += W) {
            const int64_t j = e / GATHER_F;
            const int c = (int)(e - j * GATHER_F);
            double v = 0.0;
            if (c >= 28) {
                v = ax[c - 28];
            } else if (ns > 0) {
                const ccdgpu_segment &s = seg[s0 + j];
                v = c < 7 ? s.magnitude[c] : c < 14 ? s.rmse[c - 7] : c < 21 ? s.coef[c - 14][0] : s.intercept[c - 21];
                v = (double)__double2float_rn(v);
            }
            x[(r0 + j) * GATHER_F + c] = v;
        }
        for (int64_t j = l; j < nr; j += W) skip[r0 + j] = ns > 0 ? 0 : 1;
    }
}

// The launch of a walk: one block of T lanes per T rows, the feature vectors and a chunk in its LDS.
template <int T, class... P, class... A>
int launch(void (*k)(P...), const CcdForestDev &f, int64_t n_rows, hipStream_t s, A... args) {
    const int lds = feat_bytes(f.n_features, T) + f.chunk_cap;
    if (lds > LDS_BYTES || f.chunk_cap < 16) return -1;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return -1;
    const int64_t blocks = (n_rows + T - 1) / T;
    if (blocks <= 0 || blocks > 0x7fffffff) return -1;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(T), lds, s, f, args...);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int N>
using Int = std::integral_constant<int, N>;

// go(Int<T>) for the forest's rows per block
template <class Go>
int with_threads(const CcdForestDev &f, Go &&go) {
    if (f.threads == 512) return go(Int<512>{});
    if (f.threads == 256) return go(Int<256>{});
    return -1;
}

// go(Int<NC>, Int<T>) for the accumulators' width -- the least of 2, 4, 9, 16, 32 that holds the
// forest's classes -- and its rows per block
template <class Go>
int with_width(const CcdForestDev &f, Go &&go) {
    return with_threads(f, [&](auto t) {
        const int nc = f.n_classes;
        if (nc <= 2) return go(Int<2>{}, t);
        if (nc <= 4) return go(Int<4>{}, t);
        if (nc <= 9) return go(Int<9>{}, t);
        if (nc <= 16) return go(Int<16>{}, t);
        return go(Int<32>{}, t);
    });
}

bool dims_ok(const CcdForestDev &f) {
    return f.n_classes >= 1 && f.n_classes <= CCDGPU_FOREST_MAX_CLASSES && f.n_features >= 1 &&
           f.n_features <= CCDGPU_FOREST_MAX_FEATURES;
}

}  // namespace

// Rows per block: 512 where the feature vectors of 512 rows leave a chunk's room in LDS (up to 35
// features), else 256 (at 33 features the 256-lane shape, two blocks and two half-size chunks per
// CU, measured 1.9x slower: DESIGN.md 6d).
extern "C" int32_t ccdk_forest_threads(int32_t n_features) {
    if (n_features < 1 || n_features > CCDGPU_FOREST_MAX_FEATURES) return 0;
    return feat_bytes(n_features, 512) + MIN_CHUNK <= LDS_BYTES ? 512 : 256;
}

// Chunk room: the CU's LDS split among the blocks that fit it (at most 2048 lanes per CU), less
// the block's feature vectors.
extern "C" int32_t ccdk_forest_chunk_cap(int32_t n_features) {
    const int t = ccdk_forest_threads(n_features);
    if (!t) return 0;
    const int fb = feat_bytes(n_features, t);
    int k = LDS_BYTES / (fb + MIN_CHUNK);
    if (k > 2048 / t) k = 2048 / t;
    if (k < 1) k = 1;
    return ((LDS_BYTES / k) & ~15) - fb;
}

extern "C" int ccdk_forest_classify(const CcdForestDev *f, const double *x, const unsigned char *skip, int64_t n_rows,
                                    float *out, void *stream) {
    if (n_rows <= 0) return 0;
    if (!dims_ok(*f)) return -1;
    return with_width(*f, [&](auto nc, auto t) {
        constexpr int NC = decltype(nc)::value, T = decltype(t)::value;
        return launch<T>(ccd_forest_classify<NC, T>, *f, n_rows, (hipStream_t)stream, x, skip, n_rows, out);
    });
}

extern "C" int ccdk_forest_oob(const CcdForestDev *f, const double *x, const uint64_t *tree_key, int64_t first_row,
                               int64_t n_rows, float *out, int32_t *n_oob, void *stream) {
    if (n_rows <= 0) return 0;
    if (!dims_ok(*f) || first_row < 0) return -1;
    return with_width(*f, [&](auto nc, auto t) {
        constexpr int NC = decltype(nc)::value, T = decltype(t)::value;
        return launch<T>(ccd_forest_oob<NC, T>, *f, n_rows, (hipStream_t)stream, x, tree_key, (uint64_t)first_row, n_rows, out,
                         n_oob);
    });
}

// (no accumulators, so no class-count widths)
extern "C" int ccdk_forest_permutation(const CcdForestDev *f, const double *x, const int32_t *labels, const uint64_t *tree_key,
                                       const uint32_t *perm_ab, int64_t n_rows, uint32_t *oob_rows, uint32_t *correct,
                                       uint32_t *lost, uint32_t *gained, void *stream) {
    if (n_rows <= 0) return 0;
    if (!dims_ok(*f) || n_rows > CCDGPU_TRAIN_MAX_ROWS) return -1;
    return with_threads(*f, [&](auto t) {
        constexpr int T = decltype(t)::value;
        return launch<T>(ccd_forest_permutation<T>, *f, n_rows, (hipStream_t)stream, x, labels, tree_key,
                         reinterpret_cast<const uint2 *>(perm_ab), n_rows, oob_rows, correct, lost, gained);
    });
}

extern "C" int ccdk_forest_gather(const ccdgpu_segment *seg, const int64_t *seg_off, const int64_t *row_off,
                                  const double *aux, int64_t n_pix, int64_t n_seg, int64_t n_rows, double *x,
                                  unsigned char *skip, void *stream) {
    if (n_pix <= 0) return 0;
    const int64_t b = (n_pix + 3) / 4;
    hipLaunchKernelGGL(ccd_forest_gather, dim3((unsigned)(b < 1024 ? b : 1024)), dim3(256), 0, (hipStream_t)stream, seg,
                       seg_off, row_off, aux, n_pix, n_seg, n_rows, x, skip);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
