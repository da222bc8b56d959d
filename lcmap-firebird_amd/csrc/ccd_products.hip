// ccd_products.hip -- MI355X (gfx950) annual change and land-cover product rasters from segments:
// per pixel and product date the time of spectral change, change magnitude, time since last change,
// spectral stability period, model quality, primary / secondary land cover with their confidences
// and the annual land-cover change.
//
// include/ccdgpu.h states the rule; these kernels reproduce it exactly.  This file is built with
// -ffp-contract=off: every product, sum and quotient of a value is rounded on its own.
//
// ccd_product_records: the work unit is a row (a table row, or a segment of a run's CSR).  A block
// takes RPB consecutive rows, reads what the products need of them cooperatively -- 16 lanes over 16
// consecutive dwords of a row (sday .. mag[6] lie together), so no lane strides a 312-byte row -- into
// LDS, then one lane per row reduces it to a 32-byte CcdProductRecord: days, flags, the change
// magnitude, and the labels and confidences of its rfrawp row.  The sqrt, the class sums and the
// divisions therefore run once per row, not once per row and date.
//
// ccd_products: lane = pixel.  A block's pixels are consecutive, so their records are one contiguous
// stretch and every product store of a wave is one contiguous run (64, 128 or 256 bytes).  The dates
// and their year windows are indexed by the date loop's counter alone, uniform over the wave, so they
// are read through the scalar cache into scalar registers.  A lane walks the dates in the order given
// and, per date, its own records, carrying the previous lcpri for lcachg.  The walk is clamped to the
// record array: no offset, however wrong, reads outside it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ccdgpu.h"
#include "ccd_products.h"

namespace {

constexpr int NB = CCDGPU_NBANDS;
constexpr int RPB = 256;  // rows a block of ccd_product_records reduces
constexpr int NF = 16;    // dwords read per row
constexpr int PT = 64;    // pixels (= threads) per block of ccd_products

// the fields of a row, as dwords of the LDS copy
enum { F_SDAY = 0, F_EDAY, F_BDAY, F_CURQA, F_HAS, F_CHPROB, F_MAG, F_END = F_MAG + NB };
static_assert(F_END <= NF, "fields per row");
static_assert(sizeof(CcdProductRecord) == 32, "CcdProductRecord layout");
static_assert(offsetof(ccdgpu_row, sday) == 8 && offsetof(ccdgpu_row, eday) == 12 && offsetof(ccdgpu_row, bday) == 16 &&
                  offsetof(ccdgpu_row, curqa) == 20 && offsetof(ccdgpu_row, has_model) == 24 &&
                  offsetof(ccdgpu_row, chprob) == 28 && offsetof(ccdgpu_row, mag) == 32 &&
                  sizeof(ccdgpu_row) >= 8 + 4 * NF,
              "ccdgpu_row layout");

// field f of a table row: dword 2 + f as stored (f >= F_END: not used)
__device__ __forceinline__ uint32_t field(const ccdgpu_row &r, int f) { return reinterpret_cast<const uint32_t *>(&r)[2 + f]; }

// the same of a run's segment: the float32 values the row packer stores (ccd_rows.hip)
__device__ __forceinline__ uint32_t field(const ccdgpu_segment &s, int f) {
    switch (f) {
    case F_SDAY: return (uint32_t)s.start_day;
    case F_EDAY: return (uint32_t)s.end_day;
    case F_BDAY: return (uint32_t)s.break_day;
    case F_CURQA: return (uint32_t)s.curve_qa;
    case F_HAS: return 1u;
    case F_CHPROB: return __float_as_uint(__double2float_rn(s.change_probability));
    default: return f < F_END ? __float_as_uint(__double2float_rn(s.magnitude[f - F_MAG])) : 0u;
    }
}

template <class M>
__global__ __launch_bounds__(RPB) void ccd_product_records(const M *__restrict__ models, int64_t n_models,
                                                           const float *__restrict__ rfrawp, int64_t n_rf_rows,
                                                           const int64_t *__restrict__ seg_off,
                                                           const int64_t *__restrict__ row_off, int64_t n_pix,
                                                           ccdgpu_product_params par, CcdProductRecord *__restrict__ rec) {
    __shared__ uint32_t sm[RPB][NF + 1];  // (+ 1: a lane per row reads a column without bank conflicts)
    const int tid = (int)threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * RPB;
    const int n = n_models - base < RPB ? (int)(n_models - base) : RPB;
    for (int i = tid; i < n * NF; i += RPB) sm[i / NF][i % NF] = field(models[base + i / NF], i % NF);
    __syncthreads();
    if (tid >= n) return;
    const uint32_t *f = sm[tid];
    CcdProductRecord o;
    o.sday = (int32_t)f[F_SDAY];
    o.eday = (int32_t)f[F_EDAY];
    o.bday = (int32_t)f[F_BDAY];
    const int32_t curqa = (int32_t)f[F_CURQA];
    const bool model = f[F_HAS] != 0u;
    const bool brk = model && __uint_as_float(f[F_CHPROB]) == 1.0f && o.bday >= 1;
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if ((par.mag_bands >> b) & 1u) {
            const double m = (double)__uint_as_float(f[F_MAG + b]);
            s = s + m * m;
        }
    const double root = sqrt(s);
    o.scmag = root == root ? __double2float_rn(root) : __uint_as_float(0x7fc00000u);
    o.flags = (model ? CCD_PREC_MODEL : 0u) | (brk ? CCD_PREC_BREAK : 0u) | ((uint32_t)(curqa < 0 ? 0 : curqa > 255 ? 255 : curqa) << 8);
    o.label1 = o.label2 = o.conf1 = o.conf2 = 0;
    o.pad[0] = o.pad[1] = 0u;
    // the row's rfrawp row: the row itself, or (segments) its place among the chip's table rows
    int64_t rr = base + tid;
    if (seg_off) {  // the pixel whose segments hold this one: the last p with seg_off[p] <= segment
        int64_t lo = 0, hi = n_pix;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (seg_off[mid] <= rr) lo = mid;
            else hi = mid;
        }
        const int64_t j = rr - seg_off[lo];
        rr = n_pix > 0 && j >= 0 && row_off[lo] + j < row_off[lo + 1] ? row_off[lo] + j : -1;
    }
    const int nc = par.n_classes;
    if (rfrawp && model && nc >= 1 && nc <= 32 && rr >= 0 && rr < n_rf_rows) {
        const float *raw = rfrawp + rr * nc;
        double S = 0.0, v1 = 0.0, v2 = 0.0;
        int i1 = -1, i2 = -1;
        bool nan = false;
        for (int k = 0; k < nc; ++k) {
            const double v = (double)raw[k];
            nan = nan || v != v;
            S = S + v;
            if (i1 < 0 || v > v1) {  // a new largest: the old one is the best of the rest (and earlier than its equals)
                v2 = v1;
                i2 = i1;
                v1 = v;
                i1 = k;
            } else if (i2 < 0 || v > v2) {
                v2 = v;
                i2 = k;
            }
        }
        if (!nan && S > 0.0 && S < __builtin_inf()) {
            o.flags |= CCD_PREC_COVER;
            const double c1 = rint(100.0 * v1 / S);
            o.label1 = par.labels[i1];
            o.conf1 = (uint8_t)(c1 < 0.0 ? 0.0 : c1 > 100.0 ? 100.0 : c1);
            if (i2 >= 0) {
                const double c2 = rint(100.0 * v2 / S);
                o.label2 = par.labels[i2];
                o.conf2 = (uint8_t)(c2 < 0.0 ? 0.0 : c2 > 100.0 ? 100.0 : c2);
            }
        }
    }
    rec[base + tid] = o;
}

__device__ __forceinline__ uint16_t days16(int64_t d) { return (uint16_t)(d > 65535 ? 65535 : d); }

__global__ __launch_bounds__(PT) void ccd_products(const CcdProductRecord *__restrict__ rec, int64_t n_rec,
                                                   const int64_t *__restrict__ off, int64_t off_base, int64_t n_pix,
                                                   const int64_t *__restrict__ win, int64_t n_dates, ccdgpu_product_params par,
                                                   struct ccdgpu_products out) {
    const int64_t p = (int64_t)blockIdx.x * PT + threadIdx.x;
    if (p >= n_pix) return;
    int64_t r0 = off[p] - off_base, r1 = off[p + 1] - off_base;
    if (r0 < 0 || r1 < r0 || r1 > n_rec) r1 = r0 = 0;  // (not reached for checked offsets)
    constexpr int64_t NONE = INT64_MIN;
    const bool span = par.cover == CCDGPU_COVER_SPAN;
    uint32_t prev = 0;
    for (int64_t i = 0; i < n_dates; ++i) {
        const int64_t t = win[i], a = win[n_dates + i], b = win[2 * n_dates + i];
        bool in_year = false, in_span = false, taken = false;
        int64_t doy = 0, g_last = NONE, g_stab = NONE, best = 0;
        uint32_t mag = 0u, mqa = 0u, cov = 0u;
        for (int64_t r = r0; r < r1; ++r) {
            const uint4 q = *reinterpret_cast<const uint4 *>(rec + r);  // sday, eday, bday, flags
            if (!(q.w & CCD_PREC_MODEL)) continue;
            const uint2 e = *reinterpret_cast<const uint2 *>(&rec[r].scmag);  // scmag; label1, label2, conf1, conf2
            const int64_t sday = (int32_t)q.x, eday = (int32_t)q.y, bday = (int32_t)q.z;
            if (q.w & CCD_PREC_BREAK) {
                if (!in_year && a <= bday && bday < b) {
                    in_year = true;
                    doy = bday - a + 1;
                    mag = e.x;
                }
                if (bday <= t) {
                    g_last = bday > g_last ? bday : g_last;
                    g_stab = bday > g_stab ? bday : g_stab;
                }
            }
            if (sday > t) continue;
            g_stab = sday > g_stab ? sday : g_stab;
            const bool holds = t <= eday;
            if (holds && !in_span) {
                in_span = true;
                mqa = (q.w >> 8) & 0xffu;
            }
            if (span ? holds && !taken : !taken || sday >= best) {
                taken = true;
                best = sday;
                cov = (q.w & CCD_PREC_COVER) ? e.y : 0u;
            }
        }
        const int64_t at = i * n_pix + p;
        if (out.sctime) out.sctime[at] = (uint16_t)doy;
        if (out.scmag) out.scmag[at] = __uint_as_float(mag);
        if (out.sclast) out.sclast[at] = g_last == NONE ? (uint16_t)0 : days16(t - g_last);
        if (out.scstab) out.scstab[at] = g_stab != NONE ? days16(t - g_stab) : t >= par.bot ? days16(t - par.bot) : (uint16_t)0;
        if (out.scmqa) out.scmqa[at] = (uint8_t)mqa;
        const uint32_t pri = cov & 0xffu;
        if (out.lcpri) out.lcpri[at] = (uint8_t)pri;
        if (out.lcsec) out.lcsec[at] = (uint8_t)((cov >> 8) & 0xffu);
        if (out.lcpconf) out.lcpconf[at] = (uint8_t)((cov >> 16) & 0xffu);
        if (out.lcsconf) out.lcsconf[at] = (uint8_t)(cov >> 24);
        if (out.lcachg) out.lcachg[at] = (uint16_t)(i > 0 && prev != 0u && pri != 0u && prev != pri ? prev * 256u + pri : 0u);
        prev = pri;
    }
}

template <class M>
int launch_records(const M *models, int64_t n_models, const float *rfrawp, int64_t n_rf_rows, const int64_t *seg_off,
                   const int64_t *row_off, int64_t n_pix, const ccdgpu_product_params *par, CcdProductRecord *rec, hipStream_t s) {
    if (n_models <= 0) return 0;
    const int64_t blocks = (n_models + RPB - 1) / RPB;
    if (blocks > 0x7fffffff || !par) return -1;
    hipLaunchKernelGGL((ccd_product_records<M>), dim3((unsigned)blocks), dim3(RPB), 0, s, models, n_models, rfrawp, n_rf_rows,
                       seg_off, row_off, n_pix, *par, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

extern "C" int64_t ccdk_products_max_pixels(void) { return (int64_t)0x7fffffff * PT; }

extern "C" int ccdk_product_records_rows(const ccdgpu_row *rows, int64_t n_rows, const float *rfrawp,
                                         const ccdgpu_product_params *params, CcdProductRecord *rec, void *stream) {
    return launch_records(rows, n_rows, rfrawp, n_rows, nullptr, nullptr, 0, params, rec, (hipStream_t)stream);
}

extern "C" int ccdk_product_records_segments(const ccdgpu_segment *seg, int64_t n_seg, const float *rfrawp, int64_t n_rf_rows,
                                             const int64_t *seg_off, const int64_t *row_off, int64_t n_pix,
                                             const ccdgpu_product_params *params, CcdProductRecord *rec, void *stream) {
    if (!seg_off || !row_off) return -1;
    return launch_records(seg, n_seg, rfrawp, n_rf_rows, seg_off, row_off, n_pix, params, rec, (hipStream_t)stream);
}

extern "C" int ccdk_products(const CcdProductRecord *rec, int64_t n_rec, const int64_t *off, int64_t off_base, int64_t n_pix,
                             const int64_t *win, int64_t n_dates, const ccdgpu_product_params *params,
                             const struct ccdgpu_products *out, void *stream) {
    if (n_pix <= 0 || n_dates <= 0) return 0;
    const int64_t blocks = (n_pix + PT - 1) / PT;
    if (blocks > 0x7fffffff || !params || !out) return -1;
    hipLaunchKernelGGL(ccd_products, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, rec, n_rec, off, off_base, n_pix,
                       win, n_dates, *params, *out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
