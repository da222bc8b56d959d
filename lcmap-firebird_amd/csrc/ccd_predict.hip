// ccd_predict.hip -- MI355X (gfx950) prediction of band values from segment models: the modelled
// surface reflectance of every pixel at dates of the caller's choosing.
//
// Reference: lcmap-pyccd ccd/models/lasso.py predict (coefficient_matrix(dates, avg_days_yr, 8) @
// coef + intercept).  include/ccdgpu.h states the rule -- basis, which row a date takes, the order
// of the sum, the two output types; these kernels reproduce it exactly.  This file is built with
// -ffp-contract=off: every product and every sum of a value is rounded on its own.
//
// ccd_predict_basis: lane = date, the [n_dates][8] basis once per call, so the trigonometry runs
// once per date and not once per pixel and date.
//
// ccd_predict: lane = date, the pixel is uniform over the block.  A block covers T consecutive dates
// and walks PPB consecutive pixels with them: a lane keeps its date's basis in registers for all of
// them, and per pixel and band the block's stores are one contiguous stretch (a wave stores 256
// contiguous bytes of float32, 128 of int16, per instruction).  A pixel's models are block-uniform
// data: the block copies them into LDS once (CCD_PREDICT_CACHE_ROWS at a time, float32 as stored or
// narrowed from the run's segments), every lane then reads the same LDS address (a broadcast).  The
// selection loop's trip count is the pixel's row count; the 7 bands are evaluated only under the
// lanes that took the row (no lane: the wave branches over the evaluation).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ccdgpu.h"
#include "ccd_predict.h"

namespace {

constexpr int T = 256;                         // dates per block
constexpr int PPB = 8;                         // pixels a block walks with its dates
constexpr int CACHE = CCD_PREDICT_CACHE_ROWS;  // models in LDS at a time
constexpr int NB = CCDGPU_NBANDS;

// what the evaluation needs of a row, as dwords: sday, eday, has_model, intercept[7], coef[7][7]
constexpr int M_DW = 3 + NB + NB * 7;
struct Model {
    int32_t sday, eday, has;
    float icpt[NB];
    float coef[NB][7];
};
static_assert(sizeof(Model) == M_DW * 4, "Model layout");
static_assert(sizeof(ccdgpu_row) % 4 == 0 && offsetof(ccdgpu_row, sday) == 8 && offsetof(ccdgpu_row, eday) == 12 &&
                  offsetof(ccdgpu_row, has_model) == 24 && offsetof(ccdgpu_row, coef) == 88 &&
                  offsetof(ccdgpu_row, intercept) == 284,
              "ccdgpu_row layout");

// dword f of the Model of a table row: copied as stored
__device__ __forceinline__ uint32_t model_dword(const ccdgpu_row &r, int f) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(&r);
    constexpr int SDAY = (int)(offsetof(ccdgpu_row, sday) / 4), EDAY = (int)(offsetof(ccdgpu_row, eday) / 4);
    constexpr int HAS = (int)(offsetof(ccdgpu_row, has_model) / 4), COEF = (int)(offsetof(ccdgpu_row, coef) / 4);
    constexpr int ICPT = (int)(offsetof(ccdgpu_row, intercept) / 4);
    return w[f == 0 ? SDAY : f == 1 ? EDAY : f == 2 ? HAS : f < 3 + NB ? ICPT + (f - 3) : COEF + (f - 3 - NB)];
}

// the same of a run's segment: the float32 value the row packer stores (ccd_rows.hip)
__device__ __forceinline__ uint32_t model_dword(const ccdgpu_segment &s, int f) {
    if (f == 0) return (uint32_t)s.start_day;
    if (f == 1) return (uint32_t)s.end_day;
    if (f == 2) return 1u;
    const double v = f < 3 + NB ? s.intercept[f - 3] : (&s.coef[0][0])[f - 3 - NB];
    return __float_as_uint(__double2float_rn(v));
}

__device__ __forceinline__ void put(float *o, double v, bool has) {
    *o = has && v == v ? __double2float_rn(v) : __uint_as_float(0x7fc00000u);
}
__device__ __forceinline__ void put(int16_t *o, double v, bool has) {
    const double r = rint(v);  // halves to even
    *o = !has || v != v ? (int16_t)-9999 : r < -32768.0 ? (int16_t)-32768 : r > 32767.0 ? (int16_t)32767 : (int16_t)(int)r;
}

__global__ __launch_bounds__(256) void ccd_predict_basis(const int64_t *__restrict__ dates, int64_t n_dates, double avg_days_yr,
                                                         double *__restrict__ basis) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_dates) return;
    const int64_t di = dates[r];
    const double w = 2.0 * M_PI / avg_days_yr;
    const double w12 = w * (double)di;
    const double w34 = 2.0 * w12;
    const double w56 = 3.0 * w12;
    double *row = basis + r * 8;
    row[0] = (double)di;
    row[1] = cos(w12);
    row[2] = sin(w12);
    row[3] = cos(w34);
    row[4] = sin(w34);
    row[5] = cos(w56);
    row[6] = sin(w56);
    row[7] = 0.0;
}

template <class M, class O>
__global__ __launch_bounds__(T) void ccd_predict(const M *__restrict__ models, const int64_t *__restrict__ off, int64_t off_base,
                                                 int64_t n_models, int64_t n_pix, const int64_t *__restrict__ dates,
                                                 const double *__restrict__ basis, int64_t n_dates, int cover,
                                                 O *__restrict__ out, int32_t *__restrict__ seg_index) {
    __shared__ Model sm[CACHE];
    const int tid = (int)threadIdx.x;
    const int64_t d = (int64_t)blockIdx.x * T + tid;
    const bool live = d < n_dates;
    double B[7];
    int64_t t = 0;
    if (live) {
        t = dates[d];
#pragma unroll
        for (int k = 0; k < 7; ++k) B[k] = basis[d * 8 + k];
    } else {
#pragma unroll
        for (int k = 0; k < 7; ++k) B[k] = 0.0;
    }
    const int64_t band_stride = n_pix * n_dates;
    const int64_t p0 = (int64_t)blockIdx.y * PPB;
    const int64_t p1 = p0 + PPB < n_pix ? p0 + PPB : n_pix;
    for (int64_t p = p0; p < p1; ++p) {
        int64_t r0 = off[p] - off_base, r1 = off[p + 1] - off_base;
        if (r0 < 0 || r1 < r0 || r1 > n_models) r1 = r0 = 0;  // (not reached for checked offsets)
        int32_t taken = -1;
        int64_t best = 0;
        double v[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) v[b] = 0.0;
        for (int64_t c0 = r0; c0 < r1; c0 += CACHE) {
            const int n = r1 - c0 < CACHE ? (int)(r1 - c0) : CACHE;
            __syncthreads();  // the previous piece (or pixel) is done with
            uint32_t *dst = reinterpret_cast<uint32_t *>(sm);
            for (int i = tid; i < n * M_DW; i += T) {
                const int j = i / M_DW;
                dst[i] = model_dword(models[c0 + j], i - j * M_DW);
            }
            __syncthreads();
            if (!live) continue;
            for (int j = 0; j < n; ++j) {
                const Model &m = sm[j];
                bool take = m.has != 0 && (int64_t)m.sday <= t;
                if (cover == CCDGPU_COVER_SPAN)
                    take = take && taken < 0 && t <= (int64_t)m.eday;
                else
                    take = take && (taken < 0 || (int64_t)m.sday >= best);
                if (take) {
                    taken = (int32_t)(c0 - r0) + j;
                    best = m.sday;
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        double a = (double)m.icpt[b];
#pragma unroll
                        for (int k = 0; k < 7; ++k) a = a + (double)m.coef[b][k] * B[k];
                        v[b] = a;
                    }
                }
            }
        }
        if (!live) continue;
        const int64_t at = p * n_dates + d;
#pragma unroll
        for (int b = 0; b < NB; ++b) put(out + b * band_stride + at, v[b], taken >= 0);
        if (seg_index) seg_index[at] = taken;
    }
}

template <class M>
int launch(const M *models, const int64_t *off, int64_t off_base, int64_t n_models, int64_t n_pix, const int64_t *dates,
           const double *basis, int64_t n_dates, int32_t cover, int32_t dtype, void *out, int32_t *seg_index, hipStream_t s) {
    if (n_pix <= 0 || n_dates <= 0) return 0;
    const int64_t bx = (n_dates + T - 1) / T, by = (n_pix + PPB - 1) / PPB;
    if (bx > 0x7fffffff || by > 65535) return -1;
    if (cover != CCDGPU_COVER_SPAN && cover != CCDGPU_COVER_EXTEND) return -1;
    const dim3 grid((unsigned)bx, (unsigned)by);
    if (dtype == CCDGPU_PREDICT_F32)
        hipLaunchKernelGGL((ccd_predict<M, float>), grid, dim3(T), 0, s, models, off, off_base, n_models, n_pix, dates, basis,
                           n_dates, cover, static_cast<float *>(out), seg_index);
    else if (dtype == CCDGPU_PREDICT_I16)
        hipLaunchKernelGGL((ccd_predict<M, int16_t>), grid, dim3(T), 0, s, models, off, off_base, n_models, n_pix, dates, basis,
                           n_dates, cover, static_cast<int16_t *>(out), seg_index);
    else
        return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

// most pixels one launch takes (grid.y of ccd_predict)
extern "C" int64_t ccdk_predict_max_pixels(void) { return (int64_t)65535 * PPB; }

extern "C" int ccdk_predict_basis(const int64_t *dates, int64_t n_dates, double avg_days_yr, double *basis, void *stream) {
    if (n_dates <= 0) return 0;
    const int64_t blocks = (n_dates + 255) / 256;
    if (blocks > 0x7fffffff) return -1;
    hipLaunchKernelGGL(ccd_predict_basis, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dates, n_dates, avg_days_yr,
                       basis);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int ccdk_predict_rows(const ccdgpu_row *rows, const int64_t *off, int64_t off_base, int64_t n_models, int64_t n_pix,
                                 const int64_t *dates, const double *basis, int64_t n_dates, int32_t cover, int32_t dtype,
                                 void *out, int32_t *seg_index, void *stream) {
    return launch(rows, off, off_base, n_models, n_pix, dates, basis, n_dates, cover, dtype, out, seg_index, (hipStream_t)stream);
}

extern "C" int ccdk_predict_segments(const ccdgpu_segment *seg, const int64_t *off, int64_t off_base, int64_t n_models,
                                     int64_t n_pix, const int64_t *dates, const double *basis, int64_t n_dates, int32_t cover,
                                     int32_t dtype, void *out, int32_t *seg_index, void *stream) {
    return launch(seg, off, off_base, n_models, n_pix, dates, basis, n_dates, cover, dtype, out, seg_index, (hipStream_t)stream);
}
