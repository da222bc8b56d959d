// ccdgpu_products.cpp -- annual change and land-cover product rasters from segments
// (include/ccdgpu.h; kernels in ccd_products.hip; the request's checks in ccdgpu_checks.cpp).
#include <algorithm>

#include "ccdgpu_host.h"

using namespace ccdhost;

// device bytes of a slab's output when the context names no pixel count
static const int64_t PRODUCT_SLAB_BYTES = (int64_t)256 << 20;

namespace {

// One requested product: where the caller wants it, its element size, and its plane in q_out.
struct Plane {
    unsigned char *host;
    int64_t esz;
    size_t at;
};

// The requested products in struct order, and the device struct over q_out for slabs of `slab` pixels.
// Returns the bytes of q_out.
size_t plan(const struct ccdgpu_products &o, int64_t slab, int64_t n_dates, Plane (&pl)[10], int &n) {
    void *const host[10] = {o.sctime, o.scmag, o.sclast, o.scstab, o.scmqa, o.lcpri, o.lcsec, o.lcpconf, o.lcsconf, o.lcachg};
    static const int64_t esz[10] = {2, 4, 2, 2, 1, 1, 1, 1, 1, 2};
    size_t at = 0;
    n = 0;
    for (int k = 0; k < 10; ++k) {
        if (!host[k]) continue;
        pl[n++] = Plane{static_cast<unsigned char *>(host[k]), esz[k], at};
        at += ((size_t)(slab * n_dates * esz[k]) + 255) & ~(size_t)255;
    }
    return at;
}

struct ccdgpu_products device_planes(const struct ccdgpu_products &o, const Plane (&pl)[10], unsigned char *base) {
    struct ccdgpu_products d = {};
    int j = 0;
    auto next = [&](const void *wanted) -> void * { return wanted ? base + pl[j++].at : nullptr; };
    d.sctime = static_cast<uint16_t *>(next(o.sctime));
    d.scmag = static_cast<float *>(next(o.scmag));
    d.sclast = static_cast<uint16_t *>(next(o.sclast));
    d.scstab = static_cast<uint16_t *>(next(o.scstab));
    d.scmqa = static_cast<uint8_t *>(next(o.scmqa));
    d.lcpri = static_cast<uint8_t *>(next(o.lcpri));
    d.lcsec = static_cast<uint8_t *>(next(o.lcsec));
    d.lcpconf = static_cast<uint8_t *>(next(o.lcpconf));
    d.lcsconf = static_cast<uint8_t *>(next(o.lcsconf));
    d.lcachg = static_cast<uint16_t *>(next(o.lcachg));
    return d;
}

}  // namespace

// Both paths, slab by slab over whole pixels.  Host table: pixel p has the rows h_off[p] .. h_off[p + 1]
// of h_rows (and of h_rf), uploaded and reduced to records per slab.  Chained (h_rows NULL): the n_seg
// segments d_seg of a chip, whose segment and row offsets make_row_offsets has put on the device
// (seg_off1, row_off) and whose n_rf_rows rfrawp rows h_rf holds; reduced to records once.
// A slab's planes come back with one copy per requested product: strided, since a slab's plane is np
// pixels wide and the caller's n_pix.
static int products_run(ccdgpu_ctx *c, const ccdgpu_row *h_rows, const ccdgpu_segment *d_seg, int64_t n_seg, const float *h_rf,
                        int64_t n_rf_rows, const int64_t *h_off, int64_t n_pix, int64_t n_dates, const int64_t *dates,
                        const ccdgpu_product_params *par, const struct ccdgpu_products *out, double *kernel_seconds) {
    HIPCHK(hipSetDevice(c->device));
    for (auto &e : c->q_ev) HIPCHK(e.create());
    int rc, n_planes = 0;
    Plane pl[10];
    (void)plan(*out, 1, n_dates, pl, n_planes);
    int64_t per_pixel = 0;
    for (int k = 0; k < n_planes; ++k) per_pixel += n_dates * pl[k].esz;
    int64_t slab = c->product_slab_pixels > 0 ? c->product_slab_pixels : std::max<int64_t>(1, PRODUCT_SLAB_BYTES / per_pixel);
    slab = std::min(slab, std::min(n_pix, ccdk_products_max_pixels()));
    const size_t out_bytes = plan(*out, slab, n_dates, pl, n_planes);
    const int64_t nc = par->n_classes;
    const bool cover = h_rf != nullptr && nc > 0;
    if ((rc = c->q_win.ensure((size_t)n_dates * 3)) || (rc = c->q_out.ensure(out_bytes)) ||
        (h_rows && (rc = c->q_off.ensure((size_t)slab + 1))))
        return rc;
    // the dates with a(t) and b(t), from a host copy that outlives the upload
    c->q_win_host.resize((size_t)n_dates * 3);
    for (int64_t i = 0; i < n_dates; ++i) {
        c->q_win_host[i] = dates[i];
        year_window(dates[i], &c->q_win_host[n_dates + i], &c->q_win_host[2 * n_dates + i]);
    }
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->q_win.p, c->q_win_host.data(), sizeof(int64_t) * (size_t)n_dates * 3, hipMemcpyHostToDevice, ax));
    const struct ccdgpu_products d_out = device_planes(*out, pl, c->q_out.p);
    double secs = 0.0;
    if (!h_rows && n_seg > 0) {  // chained: the chip's records once
        if ((rc = c->q_rec.ensure((size_t)n_seg)) || (cover && n_rf_rows > 0 && (rc = c->q_rf.ensure((size_t)(n_rf_rows * nc))))) {
            (void)hipStreamSynchronize(ax);
            return rc;
        }
        if (cover && n_rf_rows > 0)
            HIPCHK(hipMemcpyAsync(c->q_rf.p, h_rf, sizeof(float) * (size_t)(n_rf_rows * nc), hipMemcpyHostToDevice, ax));
    }
    for (int64_t p0 = 0; p0 < n_pix; p0 += slab) {
        const int64_t np = std::min(slab, n_pix - p0);
        const int64_t r0 = h_off[p0], nr = h_off[p0 + np] - r0;
        int bad = 0;
        if (h_rows) {
            HIPCHK(hipMemcpyAsync(c->q_off.p, h_off + p0, sizeof(int64_t) * (size_t)(np + 1), hipMemcpyHostToDevice, ax));
            if (nr > 0) {
                if ((rc = c->q_rows.ensure((size_t)nr)) || (rc = c->q_rec.ensure((size_t)nr)) ||
                    (cover && (rc = c->q_rf.ensure((size_t)(nr * nc))))) {
                    (void)hipStreamSynchronize(ax);
                    return rc;
                }
                HIPCHK(hipMemcpyAsync(c->q_rows.p, h_rows + r0, sizeof(ccdgpu_row) * (size_t)nr, hipMemcpyHostToDevice, ax));
                if (cover)
                    HIPCHK(hipMemcpyAsync(c->q_rf.p, h_rf + r0 * nc, sizeof(float) * (size_t)(nr * nc), hipMemcpyHostToDevice, ax));
            }
            HIPCHK(hipEventRecord(c->q_ev[0], ax));
            bad = ccdk_product_records_rows(c->q_rows.p, nr, cover ? c->q_rf.p : nullptr, par, c->q_rec.p, ax);
            if (!bad) bad = ccdk_products(c->q_rec.p, nr, c->q_off.p, r0, np, c->q_win.p, n_dates, par, &d_out, ax);
        } else {
            HIPCHK(hipEventRecord(c->q_ev[0], ax));
            if (p0 == 0)
                bad = ccdk_product_records_segments(d_seg, n_seg, cover && n_rf_rows > 0 ? c->q_rf.p : nullptr, n_rf_rows,
                                                    c->seg_off1.p, c->row_off.p, n_pix, par, c->q_rec.p, ax);
            if (!bad) bad = ccdk_products(c->q_rec.p, n_seg, c->seg_off1.p + p0, 0, np, c->q_win.p, n_dates, par, &d_out, ax);
        }
        if (bad) {
            (void)hipStreamSynchronize(ax);
            return fail(CCDGPU_EHIP, "products kernel launch failed");
        }
        HIPCHK(hipEventRecord(c->q_ev[1], ax));
        for (int k = 0; k < n_planes; ++k) {
            const size_t e = (size_t)pl[k].esz;
            unsigned char *dst = pl[k].host + (size_t)p0 * e;
            if (np == n_pix)
                HIPCHK(hipMemcpyAsync(dst, c->q_out.p + pl[k].at, (size_t)(np * n_dates) * e, hipMemcpyDeviceToHost, ax));
            else
                HIPCHK(hipMemcpy2DAsync(dst, (size_t)n_pix * e, c->q_out.p + pl[k].at, (size_t)np * e, (size_t)np * e,
                                        (size_t)n_dates, hipMemcpyDeviceToHost, ax));
        }
        HIPCHK(hipStreamSynchronize(ax));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->q_ev[0], c->q_ev[1]);
        secs += ms * 1e-3;
    }
    if (kernel_seconds) *kernel_seconds = secs;
    return 0;
}

extern "C" {

int ccdgpu_products(ccdgpu_ctx *c, int64_t n_pix, const int64_t *row_offsets, const ccdgpu_row *rows, const float *rfrawp,
                    int64_t n_dates, const int64_t *dates, const ccdgpu_product_params *params,
                    const struct ccdgpu_products *out, double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if (n_pix < 0) return fail(CCDGPU_EINVAL, "products: n_pix must be >= 0, got " + std::to_string(n_pix));
    if (!row_offsets) return fail(CCDGPU_EINVAL, "products: row_offsets is NULL");
    if ((rc = ccdgpu_products_check(n_pix, row_offsets, row_offsets[n_pix], rows, rfrawp, n_dates, dates, params, out))) return rc;
    if (n_pix == 0 || n_dates == 0) return 0;
    return products_run(c, rows, nullptr, 0, rfrawp, 0, row_offsets, n_pix, n_dates, dates, params, out, kernel_seconds);
}

int ccdgpu_products_rows(ccdgpu_ctx *c, int32_t chip, const float *rfrawp, int64_t n_dates, const int64_t *dates,
                         const ccdgpu_product_params *params, const struct ccdgpu_products *out, double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if (!c->ran || c->shape.n_chips() <= 0) return fail(CCDGPU_EINVAL, "no completed run to make products from");
    const int64_t total = c->shape.total_pix();
    if ((int64_t)c->h_offsets.size() < total + 1) return fail(CCDGPU_EINVAL, "no completed run to make products from");
    if (chip < 0 || chip >= c->shape.n_chips())
        return fail(CCDGPU_EINVAL, "products_rows: chip " + std::to_string(chip) + " is outside [0, " +
                                       std::to_string(c->shape.n_chips()) + ")");
    if ((rc = products_check_dates(n_dates, dates)) || (rc = products_check_params(params, rfrawp, out))) return rc;
    if (n_dates == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    // the chip's segment and row offsets, relative to its first pixel: on the host (h_fo) and the device
    const int64_t p0 = c->shape.pix_off[chip], np = c->shape.npix[chip];
    int64_t n_rows = 0;
    if ((rc = make_row_offsets(c, p0, np, true, &n_rows))) return rc;
    const int64_t *soff = reinterpret_cast<const int64_t *>(c->h_fo.p);
    return products_run(c, nullptr, c->csr.p + c->h_offsets[p0], soff[np], rfrawp, n_rows, soff, np, n_dates, dates, params, out,
                        kernel_seconds);
}

int ccdgpu_chip_row_count(ccdgpu_ctx *c, int32_t chip, int64_t *n_rows) {
    if (!n_rows) return fail(CCDGPU_EINVAL, "NULL argument");
    *n_rows = 0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if (!c->ran || c->shape.n_chips() <= 0 || (int64_t)c->h_offsets.size() < c->shape.total_pix() + 1)
        return fail(CCDGPU_EINVAL, "no completed run to count rows of");
    if (chip < 0 || chip >= c->shape.n_chips())
        return fail(CCDGPU_EINVAL, "chip_row_count: chip " + std::to_string(chip) + " is outside [0, " +
                                       std::to_string(c->shape.n_chips()) + ")");
    const int64_t p0 = c->shape.pix_off[chip], np = c->shape.npix[chip];
    for (int64_t p = p0; p < p0 + np; ++p) *n_rows += std::max<int64_t>(1, c->h_offsets[p + 1] - c->h_offsets[p]);
    return 0;
}

}  // extern "C"
