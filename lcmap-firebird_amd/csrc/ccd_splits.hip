// ccd_splits.hip -- the random forest's bin edges on the device (include/ccdgpu.h states the rule in
// its position form; the host loop over feature groups and upload slabs is ccdgpu_splits.cpp).
//
// Per group of G features, with the column as the grid's y dimension throughout:
//   ccd_splits_keys       a slab of row-major x becomes feature-major uint64 keys that order as the
//                         doubles do, through a transposing LDS tile (both sides coalesced).
//   ccd_splits_ghist      every column's digit counts of all 8 passes in one read: they say which
//                         passes a column skips (all its keys share the digit) and where each digit's
//                         run begins, so no pass has to add up its own tiles first.
//   per radix pass (8 bits, least significant first), for the columns that do not skip it:
//   ccd_splits_tile_hist  per-tile digit counts in LDS -> counts [digit][tile]
//   ccd_splits_scan       one wave per digit row: the digit's base plus the running sum over the tiles
//   ccd_splits_scatter    stable within the tile: equal digits are ranked in the wave by ballot and
//                         across the block's waves by per-wave digit counts in LDS
//   then over the sorted columns:
//   ccd_splits_bcount / _bscan / _bwrite   mark the boundaries, scan their counts per tile, lay the
//                         positions down in order (into the column's free key buffer)
//   ccd_splits_walk       one wave per column walks the rule with its exact predicate, 64 boundaries
//                         per ballot, forms the midpoints and drops the non-increasing ones.
// All counters are integers, the only floating-point operations are the rule's own, and no block waits
// for another: the result does not depend on launch shapes.
#include <hip/hip_runtime.h>

#include "ccd_splits.h"

namespace {

constexpr int T = 256;
constexpr int WAVES = T / 64;
constexpr int ITEMS = CCD_SPLITS_TILE / T;  // keys per lane
constexpr int KEY_ROWS = 64;                // rows one block of ccd_splits_keys transposes
constexpr int ND = CCD_SPLITS_DIGITS;

static_assert(ND == T, "one lane per digit");

__device__ __forceinline__ uint64_t key_of(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v + 0.0);  // (-0.0 + 0.0 is +0.0)
    return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}
__device__ __forceinline__ double value_of(uint64_t k) {
    const uint64_t b = (k >> 63) ? k ^ 0x8000000000000000ull : ~k;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ uint64_t lanes_below(int lane) { return ((uint64_t)1 << lane) - 1; }
// inclusive prefix sum over the wave's lanes (every lane of the wave calls it)
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

__global__ __launch_bounds__(T) void ccd_splits_keys(const double *__restrict__ x, int64_t r0, int64_t n, int64_t n_rows,
                                                     int32_t nf, int32_t f0, int32_t G, uint64_t *__restrict__ keys) {
    extern __shared__ __align__(8) unsigned char smem[];
    uint64_t *ks = reinterpret_cast<uint64_t *>(smem);  // [G][KEY_ROWS + 1]
    constexpr int KS = KEY_ROWS + 1;
    const int64_t row0 = (int64_t)blockIdx.x * KEY_ROWS;
    if (row0 >= n) return;
    const int nrow = n - row0 < KEY_ROWS ? (int)(n - row0) : KEY_ROWS;
    const double *xb = x + row0 * nf;
    for (int i = threadIdx.x; i < nrow * nf; i += T) {
        const int r = i / nf, c = i - r * nf - f0;
        if ((unsigned)c < (unsigned)G) ks[c * KS + r] = key_of(xb[i]);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < G * KEY_ROWS; j += T) {
        const int c = j / KEY_ROWS, r = j - c * KEY_ROWS;
        if (r < nrow) keys[(size_t)c * (size_t)n_rows + (size_t)(r0 + row0 + r)] = ks[c * KS + r];
    }
}

__global__ __launch_bounds__(T) void ccd_splits_ghist(CcdSplitsGroup g) {
    __shared__ uint32_t h[CCD_SPLITS_PASSES * ND];
    const int col = blockIdx.y;
    for (int i = threadIdx.x; i < CCD_SPLITS_PASSES * ND; i += T) h[i] = 0u;
    __syncthreads();
    const uint64_t *k = g.keys[0] + (size_t)col * (size_t)g.n_rows;
    const int64_t base = (int64_t)blockIdx.x * CCD_SPLITS_TILE + threadIdx.x;
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t i = base + (int64_t)j * T;
        if (i < g.n_rows) {
            const uint64_t key = k[i];
#pragma unroll
            for (int p = 0; p < CCD_SPLITS_PASSES; ++p) (void)atomicAdd(&h[p * ND + (int)((key >> (8 * p)) & 255u)], 1u);
        }
    }
    __syncthreads();
    uint32_t *out = g.ghist + (size_t)col * CCD_SPLITS_PASSES * ND;
    for (int i = threadIdx.x; i < CCD_SPLITS_PASSES * ND; i += T) {
        const uint32_t v = h[i];
        if (v) (void)atomicAdd(out + i, v);
    }
}

__global__ __launch_bounds__(T) void ccd_splits_tile_hist(CcdSplitsGroup g, int32_t pass) {
    __shared__ uint32_t h[ND];
    const int col = blockIdx.y;
    const int src = g.plan[pass * g.n_group + col];
    if (src < 0) return;  // (the whole block)
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t *k = g.keys[src] + (size_t)col * (size_t)g.n_rows;
    const int64_t base = (int64_t)blockIdx.x * CCD_SPLITS_TILE + threadIdx.x;
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t i = base + (int64_t)j * T;
        if (i < g.n_rows) (void)atomicAdd(&h[(int)((k[i] >> (8 * pass)) & 255u)], 1u);
    }
    __syncthreads();
    g.counts[((size_t)col * ND + threadIdx.x) * (size_t)g.n_tiles + blockIdx.x] = h[threadIdx.x];
}

// grid (ND / WAVES, G): wave w of block b turns row d = b * WAVES + w of counts [d][tile] into the
// offsets of digit d's keys, tile by tile: the keys of lower digits (ghist) plus the tiles before
__global__ __launch_bounds__(T) void ccd_splits_scan(CcdSplitsGroup g, int32_t pass) {
    __shared__ uint32_t base[ND];
    __shared__ uint32_t wave_total[WAVES];
    const int col = blockIdx.y;
    if (g.plan[pass * g.n_group + col] < 0) return;  // (the whole block)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t v = g.ghist[((size_t)col * CCD_SPLITS_PASSES + pass) * ND + threadIdx.x];
    const uint32_t incl = wave_inclusive(v, lane);
    if (lane == 63) wave_total[w] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int i = 0; i < w; ++i) before += wave_total[i];
    base[threadIdx.x] = before + incl - v;
    __syncthreads();
    const int d = blockIdx.x * WAVES + w;
    uint32_t *row = g.counts + ((size_t)col * ND + d) * (size_t)g.n_tiles;
    uint32_t run = base[d];
    for (int32_t c = 0; c < g.n_tiles; c += 64) {
        const int32_t i = c + lane;
        const uint32_t t = i < g.n_tiles ? row[i] : 0u;
        const uint32_t s = wave_inclusive(t, lane);
        if (i < g.n_tiles) row[i] = run + s - t;
        run += __shfl(s, 63, 64);
    }
}

// A tile's keys in the order the scatter keeps: wave w, item j, lane l is key w * 64 * ITEMS + j * 64 + l.
__global__ __launch_bounds__(T) void ccd_splits_scatter(CcdSplitsGroup g, int32_t pass) {
    __shared__ uint32_t wcount[WAVES * ND];
    const int col = blockIdx.y;
    const int src = g.plan[pass * g.n_group + col];
    if (src < 0) return;  // (the whole block)
    const uint64_t *in = g.keys[src] + (size_t)col * (size_t)g.n_rows;
    uint64_t *out = g.keys[src ^ 1] + (size_t)col * (size_t)g.n_rows;
    for (int i = threadIdx.x; i < WAVES * ND; i += T) wcount[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t below = lanes_below(lane);
    const int64_t first = (int64_t)blockIdx.x * CCD_SPLITS_TILE + (int64_t)w * 64 * ITEMS + lane;
    volatile uint32_t *mine = wcount + w * ND;  // this wave's digit counts so far
    uint64_t key[ITEMS];
    uint32_t rank[ITEMS];
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t i = first + (int64_t)j * 64;
        const bool valid = i < g.n_rows;
        key[j] = valid ? in[i] : 0ull;
        const uint32_t d = (uint32_t)(key[j] >> (8 * pass)) & 255u;
        uint64_t peers = __ballot(valid);  // the lanes of this item with the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t pre = mine[d];
        rank[j] = pre + (uint32_t)__popcll(peers & below);
        __builtin_amdgcn_wave_barrier();
        if (valid && (peers & below) == 0ull) mine[d] = pre + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {  // lane = digit: where each wave's keys of the digit begin
        uint32_t at = g.counts[((size_t)col * ND + threadIdx.x) * (size_t)g.n_tiles + blockIdx.x];
        for (int i = 0; i < WAVES; ++i) {
            const uint32_t t = wcount[i * ND + threadIdx.x];
            wcount[i * ND + threadIdx.x] = at;
            at += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t i = first + (int64_t)j * 64;
        if (i < g.n_rows) {
            const uint32_t d = (uint32_t)(key[j] >> (8 * pass)) & 255u;
            const uint32_t to = wcount[w * ND + d] + rank[j];
            if ((int64_t)to < g.n_rows) out[to] = key[j];
        }
    }
}

// the sorted keys of column col, and its free buffer as the boundary positions
__device__ __forceinline__ const uint64_t *sorted_keys(const CcdSplitsGroup &g, int col) {
    return g.keys[g.sorted_in[col]] + (size_t)col * (size_t)g.n_rows;
}
__device__ __forceinline__ int32_t *positions(const CcdSplitsGroup &g, int col) {
    return reinterpret_cast<int32_t *>(g.keys[g.sorted_in[col] ^ 1] + (size_t)col * (size_t)g.n_rows);
}

__global__ __launch_bounds__(T) void ccd_splits_bcount(CcdSplitsGroup g) {
    __shared__ uint32_t wave_total[WAVES];
    const int col = blockIdx.y;
    const uint64_t *s = sorted_keys(g, col);
    const int64_t base = (int64_t)blockIdx.x * CCD_SPLITS_TILE + threadIdx.x;
    uint32_t c = 0;
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t i = base + (int64_t)j * T;
        if (i >= 1 && i < g.n_rows) c += s[i] != s[i - 1];
    }
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < WAVES; ++i) t += wave_total[i];
        g.bcount[(size_t)col * (g.n_tiles + 1) + blockIdx.x] = t;
    }
}

// one wave per column: bcount [0 .. n_tiles) becomes its exclusive prefix sum, [n_tiles] the total
__global__ __launch_bounds__(64) void ccd_splits_bscan(CcdSplitsGroup g) {
    const int lane = threadIdx.x;
    uint32_t *row = g.bcount + (size_t)blockIdx.x * (g.n_tiles + 1);
    uint32_t run = 0;
    for (int32_t c = 0; c < g.n_tiles; c += 64) {
        const int32_t i = c + lane;
        const uint32_t t = i < g.n_tiles ? row[i] : 0u;
        const uint32_t s = wave_inclusive(t, lane);
        if (i < g.n_tiles) row[i] = run + s - t;
        run += __shfl(s, 63, 64);
    }
    if (lane == 0) row[g.n_tiles] = run;
}

__global__ __launch_bounds__(T) void ccd_splits_bwrite(CcdSplitsGroup g) {
    __shared__ uint32_t wave_total[WAVES];
    const int col = blockIdx.y;
    const uint64_t *s = sorted_keys(g, col);
    int32_t *pos = positions(g, col);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t below = lanes_below(lane);
    const int64_t first = (int64_t)blockIdx.x * CCD_SPLITS_TILE + (int64_t)w * 64 * ITEMS + lane;
    uint32_t flags = 0, total = 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t i = first + (int64_t)j * 64;
        const bool f = i >= 1 && i < g.n_rows && s[i] != s[i - 1];
        total += (uint32_t)__popcll(__ballot(f));
        flags |= (uint32_t)f << j;
    }
    if (lane == 0) wave_total[w] = total;
    __syncthreads();
    uint32_t at = g.bcount[(size_t)col * (g.n_tiles + 1) + blockIdx.x];
    for (int i = 0; i < w; ++i) at += wave_total[i];
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const bool f = (flags >> j) & 1u;
        const uint64_t b = __ballot(f);
        const uint32_t to = at + (uint32_t)__popcll(b & below);
        if (f && (int64_t)to < g.n_rows) pos[to] = (int32_t)(first + (int64_t)j * 64);
        at += (uint32_t)__popcll(b);
    }
}

// One wave per column.  Lane i ends up with the position of the i-th boundary whose midpoint is a
// candidate edge (at most CCDGPU_TRAIN_MAX_EDGES = 63 of them).
__global__ __launch_bounds__(64) void ccd_splits_walk(CcdSplitsGroup g, int32_t max_bins, double *__restrict__ edges,
                                                      int32_t *__restrict__ n_edges) {
    const int col = blockIdx.x, lane = threadIdx.x;
    const uint64_t *s = sorted_keys(g, col);
    const int32_t *pos = positions(g, col);
    const int32_t n = (int32_t)g.n_rows;
    const int32_t nb = (int32_t)g.bcount[(size_t)col * (g.n_tiles + 1) + g.n_tiles];
    int32_t mine = 0, cnt = 0;
    if (nb <= max_bins - 1) {  // few distinct values: every boundary
        cnt = nb;
        if (lane < nb) mine = pos[lane];
    } else {
        const double stride = (double)n / (double)max_bins;
        double target = stride;
        int32_t i = 0;  // the boundaries before i are decided
        while (i < nb && cnt < CCDGPU_TRAIN_MAX_EDGES) {
            // a boundary whose successor is not above the target is never taken: go to the first one
            // whose successor is, by a 64-way search (the successors ascend)
            int32_t lo = i, hi = nb;
            while (lo < hi) {
                const int32_t step = (hi - lo + 63) >> 6;
                const int32_t k = lo + lane * step;
                bool above = true;  // (past the range: as if above)
                if (k < hi) above = (double)(k + 1 < nb ? pos[k + 1] : n) > target;
                const uint64_t b = __ballot(above);
                if (b == 0ull) {
                    lo += 63 * step + 1;
                } else {
                    const int32_t first = (int32_t)__builtin_ctzll(b);
                    if (lo + first * step < hi) hi = lo + first * step;
                    if (first > 0) lo += (first - 1) * step + 1;
                }
            }
            i = lo;
            if (i >= nb) break;
            const int32_t k = i + lane;
            bool take = false;
            int32_t p = 0;
            if (k < nb) {
                p = pos[k];
                const int32_t next = k + 1 < nb ? pos[k + 1] : n;
                take = fabs((double)p - target) < fabs((double)next - target);
            }
            const uint64_t b = __ballot(take);
            if (b == 0ull) {
                i += 64;
                continue;
            }
            const int32_t first = (int32_t)__builtin_ctzll(b);
            const int32_t taken = __shfl(p, first, 64);
            if (lane == cnt) mine = taken;
            ++cnt;
            target += stride;
            i += first + 1;
        }
    }
    const bool have = lane < cnt && mine >= 1 && mine < n;
    double mid = 0.0;
    if (have) mid = (value_of(s[mine - 1]) + value_of(s[mine])) / 2.0;
    const double prev = __shfl_up(mid, 1, 64);
    const bool keep = have && (lane == 0 || mid > prev);
    const uint64_t kept = __ballot(keep);
    if (keep) edges[(size_t)col * CCDGPU_TRAIN_MAX_EDGES + __popcll(kept & lanes_below(lane))] = mid;
    if (lane == 0) n_edges[col] = (int32_t)__popcll(kept);
}

bool tile_grid(const CcdSplitsGroup *g, dim3 *grid) {
    if (g->n_rows <= 0 || g->n_rows > CCDGPU_TRAIN_MAX_ROWS || g->n_group <= 0 || g->n_group > CCDGPU_FOREST_MAX_FEATURES ||
        (int64_t)g->n_tiles != (g->n_rows + CCD_SPLITS_TILE - 1) / CCD_SPLITS_TILE)
        return false;
    *grid = dim3((unsigned)g->n_tiles, (unsigned)g->n_group);
    return true;
}

}  // namespace

extern "C" int ccdk_splits_keys(const CcdSplitsGroup *g, const double *x, int64_t r0, int64_t n, int32_t n_features, int32_t f0,
                                void *stream) {
    dim3 grid;
    if (n <= 0) return 0;
    if (!tile_grid(g, &grid) || r0 < 0 || r0 + n > g->n_rows || f0 < 0 || f0 + g->n_group > n_features ||
        n_features > CCDGPU_FOREST_MAX_FEATURES)
        return -1;
    const int64_t blocks = (n + KEY_ROWS - 1) / KEY_ROWS;
    if (blocks > 0x7fffffff) return -1;
    const size_t lds = sizeof(uint64_t) * (size_t)g->n_group * (KEY_ROWS + 1);
    hipLaunchKernelGGL(ccd_splits_keys, dim3((unsigned)blocks), dim3(T), lds, (hipStream_t)stream, x, r0, n, g->n_rows,
                       n_features, f0, g->n_group, g->keys[0]);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int ccdk_splits_ghist(const CcdSplitsGroup *g, void *stream) {
    dim3 grid;
    if (!tile_grid(g, &grid)) return -1;
    const size_t bytes = sizeof(uint32_t) * (size_t)g->n_group * CCD_SPLITS_PASSES * ND;
    if (hipMemsetAsync(g->ghist, 0, bytes, (hipStream_t)stream) != hipSuccess) return -1;
    hipLaunchKernelGGL(ccd_splits_ghist, grid, dim3(T), 0, (hipStream_t)stream, *g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int ccdk_splits_pass(const CcdSplitsGroup *g, int32_t pass, void *stream) {
    dim3 grid;
    if (!tile_grid(g, &grid) || pass < 0 || pass >= CCD_SPLITS_PASSES) return -1;
    hipLaunchKernelGGL(ccd_splits_tile_hist, grid, dim3(T), 0, (hipStream_t)stream, *g, pass);
    hipLaunchKernelGGL(ccd_splits_scan, dim3(ND / WAVES, (unsigned)g->n_group), dim3(T), 0, (hipStream_t)stream, *g, pass);
    hipLaunchKernelGGL(ccd_splits_scatter, grid, dim3(T), 0, (hipStream_t)stream, *g, pass);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int ccdk_splits_edges(const CcdSplitsGroup *g, int32_t max_bins, double *edges, int32_t *n_edges, void *stream) {
    dim3 grid;
    if (!tile_grid(g, &grid) || max_bins < 2 || max_bins > CCDGPU_TRAIN_MAX_EDGES + 1) return -1;
    hipLaunchKernelGGL(ccd_splits_bcount, grid, dim3(T), 0, (hipStream_t)stream, *g);
    hipLaunchKernelGGL(ccd_splits_bscan, dim3((unsigned)g->n_group), dim3(64), 0, (hipStream_t)stream, *g);
    hipLaunchKernelGGL(ccd_splits_bwrite, grid, dim3(T), 0, (hipStream_t)stream, *g);
    hipLaunchKernelGGL(ccd_splits_walk, dim3((unsigned)g->n_group), dim3(64), 0, (hipStream_t)stream, *g, max_bins, edges,
                       n_edges);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
