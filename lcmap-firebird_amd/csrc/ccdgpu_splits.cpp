// ccdgpu_splits.cpp -- the random forest's bin edges on the device (include/ccdgpu.h states the rule
// in its position form; kernels in ccd_splits.hip; the request's checks in ccdgpu_checks.cpp).
//
// The features are sorted in groups: a group's two key buffers, [G][n_rows] uint64 each, stay within
// SPLITS_GROUP_BYTES (one feature's pair where n_rows alone exceeds it).  Per group x goes up in the
// slabs training uses and every slab's columns of the group become keys; one read of the keys gives
// every column's digit counts of all 8 passes, from which the host plans the passes -- a column skips
// a pass in which all its keys share the digit, and a pass every column skips is not launched; then
// the passes, the boundaries and the walk, and the group's edges come back.
#include <algorithm>
#include <cstdlib>

#include "ccd_splits.h"
#include "ccdgpu_host.h"

using namespace ccdhost;

namespace {

// rows per upload of x (the slab of ccdgpu_train.cpp)
const int64_t SPLITS_SLAB_ROWS = (int64_t)1 << 20;
// device bytes the two key buffers of a group of features may take
const int64_t SPLITS_GROUP_BYTES = (int64_t)1 << 31;

}  // namespace

extern "C" int ccdgpu_forest_find_splits(ccdgpu_ctx *c, const double *x, int64_t n_rows, int32_t n_features, int32_t max_bins,
                                         double *edges, int32_t *n_edges, double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if ((rc = splits_validate(x, n_rows, n_features, max_bins))) return rc;
    if (!edges) return fail(CCDGPU_EINVAL, "splits: edges is NULL");
    if (!n_edges) return fail(CCDGPU_EINVAL, "splits: n_edges is NULL");
    const int32_t nf = n_features;
    std::fill(edges, edges + (size_t)nf * CCDGPU_TRAIN_MAX_EDGES, 0.0);
    std::fill(n_edges, n_edges + nf, 0);
    if (n_rows == 0) return 0;

    int64_t group = SPLITS_GROUP_BYTES / (2 * (int64_t)sizeof(uint64_t) * n_rows);
    if (const char *e = std::getenv("CCDGPU_SPLITS_GROUP_FEATURES")) group = std::atoll(e);
    group = std::max<int64_t>(1, std::min<int64_t>(group, nf));
    const int32_t n_tiles = (int32_t)((n_rows + CCD_SPLITS_TILE - 1) / CCD_SPLITS_TILE);
    const size_t hist_n = (size_t)CCD_SPLITS_PASSES * CCD_SPLITS_DIGITS;

    HIPCHK(hipSetDevice(c->device));
    hipStream_t ax = c->aux;
    DevBuf<uint64_t> d_keys[2];
    DevBuf<double> d_x, d_edges;
    DevBuf<uint32_t> d_ghist, d_counts, d_bcount;
    DevBuf<int8_t> d_plan;
    DevBuf<int32_t> d_n_edges;
    Event ev[2];
    for (auto &e : ev) HIPCHK(e.create());
    if ((rc = d_keys[0].ensure((size_t)group * (size_t)n_rows)) || (rc = d_keys[1].ensure((size_t)group * (size_t)n_rows)) ||
        (rc = d_x.ensure((size_t)(std::min(n_rows, SPLITS_SLAB_ROWS) * nf))) ||
        (rc = d_edges.ensure((size_t)group * CCDGPU_TRAIN_MAX_EDGES)) || (rc = d_n_edges.ensure((size_t)group)) ||
        (rc = d_ghist.ensure((size_t)group * hist_n)) || (rc = d_counts.ensure((size_t)group * CCD_SPLITS_DIGITS * n_tiles)) ||
        (rc = d_bcount.ensure((size_t)group * ((size_t)n_tiles + 1))) ||
        (rc = d_plan.ensure((size_t)(CCD_SPLITS_PASSES + 1) * (size_t)group)))
        return rc;
    double secs = 0.0;
    auto elapsed = [&]() {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        secs += ms * 1e-3;
    };
    auto launch_failed = [&]() {
        (void)hipStreamSynchronize(ax);
        return fail(CCDGPU_EHIP, "splits kernel launch failed");
    };

    std::vector<uint32_t> ghist;
    std::vector<int8_t> plan;  // [CCD_SPLITS_PASSES][G], then the columns' final buffers [G]
    for (int32_t f0 = 0; f0 < nf; f0 += (int32_t)group) {
        const int32_t ng = (int32_t)std::min<int64_t>(group, nf - f0);
        CcdSplitsGroup g{};
        g.keys[0] = d_keys[0].p;
        g.keys[1] = d_keys[1].p;
        g.n_rows = n_rows;
        g.n_group = ng;
        g.n_tiles = n_tiles;
        g.ghist = d_ghist.p;
        g.counts = d_counts.p;
        g.plan = d_plan.p;
        g.sorted_in = d_plan.p + (size_t)CCD_SPLITS_PASSES * ng;
        g.bcount = d_bcount.p;
        // keys, slab by slab
        for (int64_t r0 = 0; r0 < n_rows; r0 += SPLITS_SLAB_ROWS) {
            const int64_t n = std::min(SPLITS_SLAB_ROWS, n_rows - r0);
            HIPCHK(hipMemcpyAsync(d_x.p, x + r0 * nf, sizeof(double) * (size_t)(n * nf), hipMemcpyHostToDevice, ax));
            HIPCHK(hipEventRecord(ev[0], ax));
            if (ccdk_splits_keys(&g, d_x.p, r0, n, nf, f0, ax)) return launch_failed();
            HIPCHK(hipEventRecord(ev[1], ax));
            HIPCHK(hipStreamSynchronize(ax));
            elapsed();
        }
        // the columns' digit counts of every pass, and from them the plan of the passes
        ghist.resize((size_t)ng * hist_n);
        HIPCHK(hipEventRecord(ev[0], ax));
        if (ccdk_splits_ghist(&g, ax)) return launch_failed();
        HIPCHK(hipEventRecord(ev[1], ax));
        HIPCHK(hipMemcpyAsync(ghist.data(), d_ghist.p, sizeof(uint32_t) * ghist.size(), hipMemcpyDeviceToHost, ax));
        HIPCHK(hipStreamSynchronize(ax));
        elapsed();
        plan.assign((size_t)(CCD_SPLITS_PASSES + 1) * ng, 0);
        bool run[CCD_SPLITS_PASSES] = {};
        for (int32_t col = 0; col < ng; ++col) {
            int8_t at = 0;  // the buffer that holds the column's keys
            for (int32_t p = 0; p < CCD_SPLITS_PASSES; ++p) {
                const uint32_t *h = &ghist[((size_t)col * CCD_SPLITS_PASSES + p) * CCD_SPLITS_DIGITS];
                const bool one_digit = std::find(h, h + CCD_SPLITS_DIGITS, (uint32_t)n_rows) != h + CCD_SPLITS_DIGITS;
                plan[(size_t)p * ng + col] = one_digit ? (int8_t)-1 : at;
                if (!one_digit) {
                    at ^= 1;
                    run[p] = true;
                }
            }
            plan[(size_t)CCD_SPLITS_PASSES * ng + col] = at;
        }
        HIPCHK(hipMemcpyAsync(d_plan.p, plan.data(), plan.size(), hipMemcpyHostToDevice, ax));
        HIPCHK(hipMemsetAsync(d_edges.p, 0, sizeof(double) * (size_t)ng * CCDGPU_TRAIN_MAX_EDGES, ax));
        HIPCHK(hipEventRecord(ev[0], ax));
        for (int32_t p = 0; p < CCD_SPLITS_PASSES; ++p)
            if (run[p] && ccdk_splits_pass(&g, p, ax)) return launch_failed();
        if (ccdk_splits_edges(&g, max_bins, d_edges.p, d_n_edges.p, ax)) return launch_failed();
        HIPCHK(hipEventRecord(ev[1], ax));
        HIPCHK(hipMemcpyAsync(edges + (size_t)f0 * CCDGPU_TRAIN_MAX_EDGES, d_edges.p,
                              sizeof(double) * (size_t)ng * CCDGPU_TRAIN_MAX_EDGES, hipMemcpyDeviceToHost, ax));
        HIPCHK(hipMemcpyAsync(n_edges + f0, d_n_edges.p, sizeof(int32_t) * (size_t)ng, hipMemcpyDeviceToHost, ax));
        HIPCHK(hipStreamSynchronize(ax));
        elapsed();
    }
    if (kernel_seconds) *kernel_seconds = secs;
    return 0;
}
