// ccdgpu_predict.cpp -- prediction of band values from segment models (include/ccdgpu.h; kernels
// in ccd_predict.hip; the request's checks in ccdgpu_checks.cpp).
#include <algorithm>
#include <cstring>

#include "ccdgpu_host.h"
#include "ccd_predict.h"

using namespace ccdhost;

// device bytes of a slab's output when the context names no pixel count
static const int64_t PREDICT_SLAB_BYTES = (int64_t)256 << 20;

// Both paths, slab by slab over whole pixels: pixel p has the models h_off[p] .. h_off[p + 1] of the
// host table h_rows (uploaded per slab) or, with h_rows NULL, of the device segments d_seg [n_seg].
// A slab's values come back as 7 copies, one per band, into the caller's [7][n_pix][n_dates].
static int predict_run(ccdgpu_ctx *c, const ccdgpu_row *h_rows, const ccdgpu_segment *d_seg, int64_t n_seg,
                       const int64_t *h_off, int64_t n_pix, int64_t n_dates, const int64_t *dates, double avg_days_yr,
                       int32_t cover, int32_t dtype, void *out, int32_t *seg_index, double *kernel_seconds) {
    HIPCHK(hipSetDevice(c->device));
    for (auto &e : c->p_ev) HIPCHK(e.create());
    int rc;
    const int64_t esz = dtype == CCDGPU_PREDICT_I16 ? 2 : 4;
    int64_t slab = c->predict_slab_pixels > 0 ? c->predict_slab_pixels
                                              : std::max<int64_t>(1, PREDICT_SLAB_BYTES / (n_dates * (CCDGPU_NBANDS * esz + 4)));
    slab = std::min(slab, std::min(n_pix, ccdk_predict_max_pixels()));
    if ((rc = c->p_dates.ensure((size_t)n_dates)) || (rc = c->p_basis.ensure((size_t)n_dates * 8)) ||
        (rc = c->p_off.ensure((size_t)slab + 1)) || (rc = c->p_out.ensure((size_t)(CCDGPU_NBANDS * slab * n_dates * esz))) ||
        (seg_index && (rc = c->p_idx.ensure((size_t)(slab * n_dates)))))
        return rc;
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->p_dates.p, dates, sizeof(int64_t) * (size_t)n_dates, hipMemcpyHostToDevice, ax));
    double secs = 0.0;
    for (int64_t p0 = 0; p0 < n_pix; p0 += slab) {
        const int64_t np = std::min(slab, n_pix - p0);
        const int64_t r0 = h_off[p0], nr = h_off[p0 + np] - r0;
        HIPCHK(hipMemcpyAsync(c->p_off.p, h_off + p0, sizeof(int64_t) * (size_t)(np + 1), hipMemcpyHostToDevice, ax));
        if (h_rows && nr > 0) {
            if ((rc = c->p_rows.ensure((size_t)nr))) {
                (void)hipStreamSynchronize(ax);
                return rc;
            }
            HIPCHK(hipMemcpyAsync(c->p_rows.p, h_rows + r0, sizeof(ccdgpu_row) * (size_t)nr, hipMemcpyHostToDevice, ax));
        }
        HIPCHK(hipEventRecord(c->p_ev[0], ax));
        int bad = p0 == 0 ? ccdk_predict_basis(c->p_dates.p, n_dates, avg_days_yr, c->p_basis.p, ax) : 0;
        int32_t *idx = seg_index ? c->p_idx.p : nullptr;
        if (!bad)
            bad = h_rows ? ccdk_predict_rows(c->p_rows.p, c->p_off.p, r0, nr, np, c->p_dates.p, c->p_basis.p, n_dates, cover, dtype,
                                             c->p_out.p, idx, ax)
                         : ccdk_predict_segments(d_seg, c->p_off.p, 0, n_seg, np, c->p_dates.p, c->p_basis.p, n_dates, cover,
                                                 dtype, c->p_out.p, idx, ax);
        if (bad) {
            (void)hipStreamSynchronize(ax);
            return fail(CCDGPU_EHIP, "predict kernel launch failed");
        }
        HIPCHK(hipEventRecord(c->p_ev[1], ax));
        const size_t band = (size_t)(np * n_dates * esz);
        for (int b = 0; b < CCDGPU_NBANDS; ++b)
            HIPCHK(hipMemcpyAsync(static_cast<unsigned char *>(out) + ((size_t)b * n_pix + p0) * n_dates * esz,
                                  c->p_out.p + (size_t)b * band, band, hipMemcpyDeviceToHost, ax));
        if (seg_index)
            HIPCHK(hipMemcpyAsync(seg_index + p0 * n_dates, c->p_idx.p, sizeof(int32_t) * (size_t)(np * n_dates),
                                  hipMemcpyDeviceToHost, ax));
        HIPCHK(hipStreamSynchronize(ax));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->p_ev[0], c->p_ev[1]);
        secs += ms * 1e-3;
    }
    if (kernel_seconds) *kernel_seconds = secs;
    return 0;
}

extern "C" {

int ccdgpu_predict(ccdgpu_ctx *c, int64_t n_pix, const int64_t *row_offsets, const ccdgpu_row *rows, int64_t n_dates,
                   const int64_t *dates, double avg_days_yr, int32_t cover, int32_t dtype, void *out, int32_t *seg_index,
                   double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if (n_pix < 0) return fail(CCDGPU_EINVAL, "predict: n_pix must be >= 0, got " + std::to_string(n_pix));
    if (!row_offsets) return fail(CCDGPU_EINVAL, "predict: row_offsets is NULL");
    if ((rc = ccdgpu_predict_check(n_pix, row_offsets, row_offsets[n_pix], rows, n_dates, dates, avg_days_yr, cover, dtype)))
        return rc;
    if (n_pix == 0 || n_dates == 0) return 0;
    if (!out) return fail(CCDGPU_EINVAL, "predict: out is NULL");
    return predict_run(c, rows, nullptr, 0, row_offsets, n_pix, n_dates, dates, avg_days_yr, cover, dtype, out, seg_index,
                       kernel_seconds);
}

int ccdgpu_predict_rows(ccdgpu_ctx *c, int32_t chip, int64_t n_dates, const int64_t *dates, double avg_days_yr, int32_t cover,
                        int32_t dtype, void *out, int32_t *seg_index, double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if (!c->ran || c->shape.n_chips() <= 0) return fail(CCDGPU_EINVAL, "no completed run to predict from");
    const int64_t total = c->shape.total_pix();
    if ((int64_t)c->h_offsets.size() < total + 1) return fail(CCDGPU_EINVAL, "no completed run to predict from");
    if (chip < 0 || chip >= c->shape.n_chips())
        return fail(CCDGPU_EINVAL, "predict_rows: chip " + std::to_string(chip) + " is outside [0, " +
                                       std::to_string(c->shape.n_chips()) + ")");
    if ((rc = predict_check_dates(n_dates, dates, avg_days_yr)) || (rc = predict_check_modes(cover, dtype))) return rc;
    if (n_dates == 0) return 0;
    if (!out) return fail(CCDGPU_EINVAL, "predict: out is NULL");
    const int64_t p0 = c->shape.pix_off[chip];
    return predict_run(c, nullptr, c->csr.p, c->h_offsets[total], c->h_offsets.data() + p0, c->shape.npix[chip], n_dates, dates,
                       avg_days_yr, cover, dtype, out, seg_index, kernel_seconds);
}

int ccdgpu_coefficient_matrix(ccdgpu_ctx *c, int64_t n_dates, const int64_t *dates, double avg_days_yr, double *basis) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if ((rc = predict_check_dates(n_dates, dates, avg_days_yr))) return rc;
    if (n_dates == 0) return 0;
    if (!basis) return fail(CCDGPU_EINVAL, "predict: basis is NULL");
    HIPCHK(hipSetDevice(c->device));
    if ((rc = c->p_dates.ensure((size_t)n_dates)) || (rc = c->p_basis.ensure((size_t)n_dates * 8))) return rc;
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->p_dates.p, dates, sizeof(int64_t) * (size_t)n_dates, hipMemcpyHostToDevice, ax));
    if (ccdk_predict_basis(c->p_dates.p, n_dates, avg_days_yr, c->p_basis.p, ax)) {
        (void)hipStreamSynchronize(ax);
        return fail(CCDGPU_EHIP, "predict kernel launch failed");
    }
    std::vector<double> b8((size_t)n_dates * 8);
    HIPCHK(hipMemcpyAsync(b8.data(), c->p_basis.p, sizeof(double) * b8.size(), hipMemcpyDeviceToHost, ax));
    HIPCHK(hipStreamSynchronize(ax));
    for (int64_t i = 0; i < n_dates; ++i) std::memcpy(basis + i * 7, b8.data() + i * 8, sizeof(double) * 7);
    return 0;
}

}  // extern "C"
