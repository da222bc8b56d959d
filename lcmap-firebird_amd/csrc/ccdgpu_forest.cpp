// ccdgpu_forest.cpp -- random-forest classification of segment rows (include/ccdgpu.h; kernels in
// ccd_forest.hip; the forest's checks and its device form in ccdgpu_checks.cpp).
#include <algorithm>
#include <numeric>

#include "ccd_train.h"
#include "ccdgpu_host.h"

using namespace ccdhost;

// rows a classification keeps on the device at a time (the host-matrix path goes slab by slab;
// a row's result does not depend on its slab)
static const int64_t FOREST_SLAB = (int64_t)1 << 20;

// What every call that walks the context's forest checks first.
static int enter(ccdgpu_ctx *c, double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (!c->has_forest) return fail(CCDGPU_EINVAL, "no forest set (ccdgpu_forest_set)");
    return busy(c);
}

// The timed part of a call: `launch` enqueues its kernels (non-zero: one did not launch) between the two forest events.
template <class Launch>
static int timed(ccdgpu_ctx *c, Launch &&launch) {
    hipStream_t ax = c->aux;
    HIPCHK(hipEventRecord(c->f_ev[0], ax));
    if (launch()) {
        (void)hipStreamSynchronize(ax);
        return fail(CCDGPU_EHIP, "forest kernel launch failed");
    }
    HIPCHK(hipEventRecord(c->f_ev[1], ax));
    return 0;
}

// The end of what was enqueued behind timed(): the seconds between its events, added to *secs.
static int finish(ccdgpu_ctx *c, double *secs) {
    HIPCHK(hipStreamSynchronize(c->aux));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->f_ev[0], c->f_ev[1]);
    if (secs) *secs += ms * 1e-3;
    return 0;
}

// The host-matrix path: x goes through f_x in slabs; launch(r0, n) enqueues the kernel of rows [r0, r0 + n), which
// leaves their predictions in f_out (to raw).  The out-of-bag walk's: keys go up first, f_noob's counts come down too.
template <class Launch>
static int by_slab(ccdgpu_ctx *c, const double *x, int64_t n_rows, float *raw, const std::vector<uint64_t> *keys,
                   int32_t *n_oob, double *kernel_seconds, Launch &&launch) {
    const int64_t nf = c->forest.n_features, nc = c->forest.n_classes;
    const int64_t slab = std::min(n_rows, FOREST_SLAB);
    int rc = c->f_x.ensure((size_t)(slab * nf));
    if (rc || (rc = c->f_out.ensure((size_t)(slab * nc))) || (n_oob && (rc = c->f_noob.ensure((size_t)slab))) ||
        (keys && (rc = c->f_keys.ensure(keys->size()))))
        return rc;
    hipStream_t ax = c->aux;
    if (keys) HIPCHK(hipMemcpyAsync(c->f_keys.p, keys->data(), sizeof(uint64_t) * keys->size(), hipMemcpyHostToDevice, ax));
    double secs = 0.0;
    for (int64_t r0 = 0; r0 < n_rows; r0 += slab) {
        const int64_t n = std::min(slab, n_rows - r0);
        HIPCHK(hipMemcpyAsync(c->f_x.p, x + r0 * nf, sizeof(double) * (size_t)(n * nf), hipMemcpyHostToDevice, ax));
        if ((rc = timed(c, [&] { return launch(r0, n); }))) return rc;
        HIPCHK(hipMemcpyAsync(raw + r0 * nc, c->f_out.p, sizeof(float) * (size_t)(n * nc), hipMemcpyDeviceToHost, ax));
        if (n_oob) HIPCHK(hipMemcpyAsync(n_oob + r0, c->f_noob.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ax));
        if ((rc = finish(c, &secs))) return rc;
    }
    if (kernel_seconds) *kernel_seconds = secs;
    return 0;
}

// the per-tree prefix of the membership hash, once per call
static std::vector<uint64_t> tree_keys(const ccdgpu_ctx *c, uint64_t seed) {
    std::vector<uint64_t> keys((size_t)c->f_n_trees);
    for (int32_t t = 0; t < c->f_n_trees; ++t) keys[t] = ccd_train_hash_a(seed, (uint64_t)t);
    return keys;
}

extern "C" {

int ccdgpu_forest_clear(ccdgpu_ctx *c) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    (void)hipSetDevice(c->device);
    c->has_forest = false;
    c->forest = CcdForestDev{};
    c->f_n_trees = 0;
    c->f_pool.release();
    c->f_tree_off.release();
    c->f_chunk_first.release();
    return 0;
}

int ccdgpu_forest_set(ccdgpu_ctx *c, const ccdgpu_forest *f) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int32_t max_depth = 0;
    int rc = forest_validate(f, &max_depth);
    if (rc) return rc;
    const int32_t nc = f->n_classes;
    const int32_t cap = ccdk_forest_chunk_cap(f->n_features);
    std::vector<unsigned char> pool;
    std::vector<int64_t> tree_off;
    std::vector<int32_t> chunk_first;
    if ((rc = forest_build(f, cap, pool, tree_off, chunk_first))) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->aux));
    c->has_forest = false;
    if ((rc = c->f_pool.ensure(pool.size())) || (rc = c->f_tree_off.ensure(tree_off.size())) ||
        (rc = c->f_chunk_first.ensure(chunk_first.size())))
        return rc;
    HIPCHK(hipMemcpy(c->f_pool.p, pool.data(), pool.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->f_tree_off.p, tree_off.data(), sizeof(int64_t) * tree_off.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->f_chunk_first.p, chunk_first.data(), sizeof(int32_t) * chunk_first.size(), hipMemcpyHostToDevice));
    for (auto &e : c->f_ev) HIPCHK(e.create());
    c->forest.pool = c->f_pool.p;
    c->forest.tree_off = c->f_tree_off.p;
    c->forest.chunk_first = c->f_chunk_first.p;
    c->forest.n_chunks = (int32_t)chunk_first.size() - 1;
    c->forest.n_features = f->n_features;
    c->forest.n_classes = nc;
    c->forest.max_depth = max_depth;
    c->forest.threads = ccdk_forest_threads(f->n_features);
    c->forest.chunk_cap = cap;
    c->f_n_trees = f->n_trees;
    c->has_forest = true;
    return 0;
}

int ccdgpu_classify(ccdgpu_ctx *c, const double *features, int64_t n_rows, float *rfrawp, double *kernel_seconds) {
    int rc = enter(c, kernel_seconds);
    if (rc) return rc;
    if (n_rows < 0) return fail(CCDGPU_EINVAL, "n_rows must be >= 0");
    if (n_rows == 0) return 0;
    if (!features || !rfrawp) return fail(CCDGPU_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    return by_slab(c, features, n_rows, rfrawp, nullptr, nullptr, kernel_seconds, [&](int64_t, int64_t n) {
        return ccdk_forest_classify(&c->forest, c->f_x.p, nullptr, n, c->f_out.p, c->aux);
    });
}

int ccdgpu_forest_oob(ccdgpu_ctx *c, const double *x, int64_t n_rows, const ccdgpu_oob_params *p, float *oob_raw, int32_t *n_oob,
                      double *kernel_seconds) {
    int rc = enter(c, kernel_seconds);
    if (rc || (rc = oob_validate(x, n_rows, p, oob_raw, n_oob))) return rc;
    if (n_rows == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    const std::vector<uint64_t> keys = tree_keys(c, p->seed);
    return by_slab(c, x, n_rows, oob_raw, &keys, n_oob, kernel_seconds, [&](int64_t r0, int64_t n) {
        return ccdk_forest_oob(&c->forest, c->f_x.p, c->f_keys.p, p->first_row + r0, n, c->f_out.p, c->f_noob.p, c->aux);
    });
}

int ccdgpu_forest_permutation(ccdgpu_ctx *c, const double *x, const int32_t *labels, int64_t n_rows,
                              const ccdgpu_permutation_params *p, int64_t *oob_rows, int64_t *correct, int64_t *lost,
                              int64_t *gained, double *kernel_seconds) {
    int rc = enter(c, kernel_seconds);
    if (rc) return rc;
    const int32_t nf = c->forest.n_features, nc = c->forest.n_classes, nt = c->f_n_trees;
    if ((rc = permutation_validate(x, labels, n_rows, nf, nc, p, oob_rows, correct, lost, gained))) return rc;
    const size_t dense = (size_t)nt * nc, sparse = dense * nf;
    std::fill(oob_rows, oob_rows + dense, (int64_t)0);
    std::fill(correct, correct + dense, (int64_t)0);
    std::fill(lost, lost + sparse, (int64_t)0);
    std::fill(gained, gained + sparse, (int64_t)0);
    if (n_rows == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    // per (tree, feature) the column's permutation: the rule's a (made coprime to n_rows) and b
    const uint64_t n = (uint64_t)n_rows;
    const std::vector<uint64_t> keys = tree_keys(c, p->seed);
    std::vector<uint32_t> ab((size_t)nt * nf * 2);
    for (int32_t t = 0; t < nt; ++t)
        for (int32_t f = 0; f < nf; ++f) {
            const uint64_t k = ccd_train_hash(p->perm_seed, (uint64_t)t, (uint64_t)f, CCDGPU_PERM_HASH_C);
            uint64_t a = (k & 0xffffffffull) % n;
            while (std::gcd(a, n) != 1) a = a + 1 == n ? 0 : a + 1;
            ab[((size_t)t * nf + f) * 2] = (uint32_t)a;
            ab[((size_t)t * nf + f) * 2 + 1] = (uint32_t)((k >> 32) % n);
        }
    std::vector<uint32_t> cnt(2 * dense + 2 * sparse);
    if ((rc = c->f_x.ensure((size_t)(n_rows * nf))) || (rc = c->f_labels.ensure((size_t)n_rows)) ||
        (rc = c->f_keys.ensure(keys.size())) || (rc = c->f_ab.ensure(ab.size())) || (rc = c->f_cnt.ensure(cnt.size())))
        return rc;
    hipStream_t ax = c->aux;
    // x whole on the device (a row's donors are anywhere in it), uploaded slab by slab
    for (int64_t r0 = 0; r0 < n_rows; r0 += FOREST_SLAB) {
        const int64_t m = std::min(FOREST_SLAB, n_rows - r0);
        HIPCHK(hipMemcpyAsync(c->f_x.p + r0 * nf, x + r0 * nf, sizeof(double) * (size_t)(m * nf), hipMemcpyHostToDevice, ax));
    }
    HIPCHK(hipMemcpyAsync(c->f_labels.p, labels, sizeof(int32_t) * (size_t)n_rows, hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(c->f_keys.p, keys.data(), sizeof(uint64_t) * keys.size(), hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(c->f_ab.p, ab.data(), sizeof(uint32_t) * ab.size(), hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemsetAsync(c->f_cnt.p, 0, sizeof(uint32_t) * cnt.size(), ax));
    uint32_t *d_oob = c->f_cnt.p, *d_correct = d_oob + dense, *d_lost = d_correct + dense, *d_gained = d_lost + sparse;
    if ((rc = timed(c, [&] {
             return ccdk_forest_permutation(&c->forest, c->f_x.p, c->f_labels.p, c->f_keys.p, c->f_ab.p, n_rows, d_oob, d_correct,
                                            d_lost, d_gained, ax);
         })))
        return rc;
    HIPCHK(hipMemcpyAsync(cnt.data(), c->f_cnt.p, sizeof(uint32_t) * cnt.size(), hipMemcpyDeviceToHost, ax));
    if ((rc = finish(c, kernel_seconds))) return rc;
    std::copy(cnt.begin(), cnt.begin() + dense, oob_rows);
    std::copy(cnt.begin() + dense, cnt.begin() + 2 * dense, correct);
    std::copy(cnt.begin() + 2 * dense, cnt.begin() + 2 * dense + sparse, lost);
    std::copy(cnt.begin() + 2 * dense + sparse, cnt.end(), gained);
    return 0;
}

int ccdgpu_classify_rows(ccdgpu_ctx *c, const double *aux, float *rfrawp, int64_t rows_cap, int64_t *n_rows,
                         double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!n_rows) return fail(CCDGPU_EINVAL, "NULL argument");
    *n_rows = 0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if (!c->ran || c->shape.n_chips() <= 0) return fail(CCDGPU_EINVAL, "no completed run to classify");
    // the rows of the run, as ccdgpu_fetch_batch_rows_into counts them: max(1, segments) per pixel
    const int64_t np = c->shape.total_pix();
    if ((int64_t)c->h_offsets.size() < np + 1) return fail(CCDGPU_EINVAL, "no completed run to classify");
    int64_t nr = 0;
    if ((rc = make_row_offsets(c, 0, np, false, &nr))) return rc;
    *n_rows = nr;
    if (!c->has_forest) return fail(CCDGPU_EINVAL, "no forest set (ccdgpu_forest_set)");
    if (c->forest.n_features != 33)
        return fail(CCDGPU_EINVAL, "classify_rows needs a forest of 33 features (ccdc.features.columns()), this one has " +
                                       std::to_string(c->forest.n_features));
    if (rows_cap < nr)
        return fail(CCDGPU_EINVAL, "classify_rows: buffer too small (need " + std::to_string(nr) + " rows)");
    if (!aux || !rfrawp) return fail(CCDGPU_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    const int64_t nc = c->forest.n_classes;
    const int64_t s0 = c->h_offsets[0], n_seg = c->h_offsets[np] - s0;
    if ((rc = c->f_aux.ensure((size_t)np * 5)) || (rc = c->f_x.ensure((size_t)nr * 33)) || (rc = c->f_skip.ensure((size_t)nr)) ||
        (rc = c->f_out.ensure((size_t)(nr * nc))) || (rc = make_row_offsets(c, 0, np, true, &nr)))
        return rc;
    hipStream_t ax = c->aux;
    HIPCHK(hipMemcpyAsync(c->f_aux.p, aux, sizeof(double) * (size_t)np * 5, hipMemcpyHostToDevice, ax));
    if ((rc = timed(c, [&] {
             return ccdk_forest_gather(c->csr.p + s0, c->seg_off1.p, c->row_off.p, c->f_aux.p, np, n_seg, nr, c->f_x.p,
                                       c->f_skip.p, ax) ||
                    ccdk_forest_classify(&c->forest, c->f_x.p, c->f_skip.p, nr, c->f_out.p, ax);
         })))
        return rc;
    HIPCHK(hipMemcpyAsync(rfrawp, c->f_out.p, sizeof(float) * (size_t)(nr * nc), hipMemcpyDeviceToHost, ax));
    return finish(c, kernel_seconds);
}

}  // extern "C"
