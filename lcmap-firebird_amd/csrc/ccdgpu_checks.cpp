// ccdgpu_checks.cpp -- the part of the host API that touches no device: the error state, the
// default parameters and the validators of parameters, shapes, transport-encoded batches, forests,
// prediction and product requests, with the product rule's year window.  The device code trusts
// what passes here, so this unit is kept free of HIP and builds with a plain C++ compiler too
// (tests/native/host_checks.cpp and product_checks.cpp run it under sanitizers).
#include "ccdgpu_checks.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "ccd_enc_layout.h"

namespace ccdhost {

namespace {

thread_local std::string g_err;

double chi2_5_cdf(double x) {
    if (x <= 0) return 0.0;
    return std::erf(std::sqrt(x / 2.0)) - std::sqrt(2.0 * x / M_PI) * std::exp(-x / 2.0) * (1.0 + x / 3.0);
}

// inverse chi-square(5) cdf (change.adjustchgthresh uses scipy chi2.ppf(pt_cg, 5))
double chi2_5_ppf(double p) {
    double lo = 0.0, hi = 400.0;
    for (int i = 0; i < 200; ++i) {
        const double mid = 0.5 * (lo + hi);
        if (chi2_5_cdf(mid) < p) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}

// "encoded batch: chip N" + what is wrong with it
int enc_fail(int32_t chip, const std::string &what) {
    return fail(CCDGPU_EINVAL, "encoded batch: chip " + std::to_string(chip) + what);
}

// the kept-offset table of a mode 1 or 2 section: a run of at most n_obs per pixel, ending at kept
int enc_check_koff(int32_t chip, const uint32_t *koff, int64_t n_pix, int64_t n_obs, int64_t kept) {
    if (koff[0] != 0 || (int64_t)koff[n_pix] != kept) return enc_fail(chip, " kept-offset table does not end at kept");
    for (int64_t q = 0; q < n_pix; ++q)
        if (koff[q + 1] < koff[q] || (int64_t)(koff[q + 1] - koff[q]) > n_obs)
            return enc_fail(chip, " kept-offset table is not a run per pixel");
    return 0;
}

}  // namespace

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int make_shape(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, Shape &s) {
    if (n_chips <= 0) return fail(CCDGPU_EINVAL, "n_chips must be > 0");
    if (!n_pix || !n_obs) return fail(CCDGPU_EINVAL, "NULL n_pix / n_obs array");
    s.npix.assign(n_pix, n_pix + n_chips);
    s.nobs.assign(n_obs, n_obs + n_chips);
    s.obs_off.assign(n_chips + 1, 0);
    s.pix_off.assign(n_chips + 1, 0);
    s.data_off.assign(n_chips + 1, 0);
    s.n_obs_max = 0;
    for (int c = 0; c < n_chips; ++c) {
        if (n_pix[c] <= 0) return fail(CCDGPU_EINVAL, "chip " + std::to_string(c) + ": n_pix must be > 0");
        if (n_obs[c] <= 0 || n_obs[c] > CCDGPU_MAX_OBS)
            return fail(CCDGPU_EINVAL, "chip " + std::to_string(c) + ": n_obs must be in [1, " + std::to_string(CCDGPU_MAX_OBS) + "]");
        s.obs_off[c + 1] = s.obs_off[c] + n_obs[c];
        s.pix_off[c + 1] = s.pix_off[c] + n_pix[c];
        s.data_off[c + 1] = s.data_off[c] + (int64_t)n_pix[c] * n_obs[c];
        s.n_obs_max = std::max(s.n_obs_max, n_obs[c]);
    }
    if (s.total_pix() >= (int64_t)1 << 31) return fail(CCDGPU_EINVAL, "more than 2^31 - 1 pixels in one batch");
    return 0;
}

int check_params(const ccdgpu_params *p) {
    if (!p) return fail(CCDGPU_EINVAL, "params is NULL");
    if (p->peek_size < 1 || p->peek_size > CCDGPU_MAX_PEEK)
        return fail(CCDGPU_EINVAL, "peek_size must be in [1, " + std::to_string(CCDGPU_MAX_PEEK) + "]");
    if (p->meow_size < 5) return fail(CCDGPU_EINVAL, "meow_size must be >= 5 (Tmask needs > 4 observations)");
    if (p->coef_min != 4 && p->coef_min != 6 && p->coef_min != 8)
        return fail(CCDGPU_EINVAL, "coefficient counts must be 4, 6 or 8");
    if ((p->coef_mid != 4 && p->coef_mid != 6 && p->coef_mid != 8) || (p->coef_max != 4 && p->coef_max != 6 && p->coef_max != 8))
        return fail(CCDGPU_EINVAL, "coefficient counts must be 4, 6 or 8");
    if (p->lasso_max_iter < 1) return fail(CCDGPU_EINVAL, "lasso_max_iter must be >= 1");
    if ((p->detection_bands & ~0x7Fu) || (p->tmask_bands & ~0x7Fu))
        return fail(CCDGPU_EINVAL, "band masks must only use bits 0..6");
    if (p->argsort_stable != 0 && p->argsort_stable != 1) return fail(CCDGPU_EINVAL, "argsort_stable must be 0 or 1");
    return 0;
}

void fill_thr_table(const ccdgpu_params &p, double *thr) {
    for (int k = 0; k <= CCDGPU_MAX_PEEK; ++k) {
        if (k <= p.peek_size) thr[k] = p.change_threshold;
        else thr[k] = chi2_5_ppf(1.0 - std::pow(1.0 - p.change_probability, (double)p.peek_size / k));
    }
}

int encoded_check(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, const uint8_t *enc, int64_t enc_bytes,
                  bool *packed) {
    *packed = false;
    bool mode1 = false;
    if (!enc || !n_pix || !n_obs || n_chips <= 0) return fail(CCDGPU_EINVAL, "NULL or empty encoded batch");
    // the encoded batch must describe exactly these chips (the decoder trusts its headers)
    if (enc_bytes < ccd_enc_table_used(n_chips) || ccd_enc_n_chips(enc) != n_chips)
        return fail(CCDGPU_EINVAL, "encoded batch: chip table does not match n_chips");
    const int64_t *off = ccd_enc_chip_off(enc), *pixo = ccd_enc_chip_pix(enc, n_chips);
    if (off[n_chips] > enc_bytes) return fail(CCDGPU_EINVAL, "encoded batch: longer than enc_bytes");
    int64_t pb = 0, db = 0;
    for (int32_t k = 0; k < n_chips; ++k) {
        if (n_pix[k] <= 0 || n_obs[k] <= 0 || n_obs[k] > CCDGPU_MAX_OBS)
            return enc_fail(k, " has no pixels / observations");
        if (off[k] < 0 || off[k] + CCD_ENC_HDR > off[k + 1] || pixo[k] != pb)
            return fail(CCDGPU_EINVAL, "encoded batch: bad chip table entry " + std::to_string(k));
        const uint8_t *sec = enc + off[k];
        const ccd_enc_hdr *h = reinterpret_cast<const ccd_enc_hdr *>(sec);
        if ((h->mode != CCD_ENC_MODE_RAW && h->mode != CCD_ENC_MODE_COLS && h->mode != CCD_ENC_MODE_PACK) ||
            h->n_pix != n_pix[k] || h->n_obs != n_obs[k] || h->data_off != db ||
            (h->mode != CCD_ENC_MODE_RAW && (h->n_pal < 1 || h->n_pal > 16)))
            return enc_fail(k, " header does not match its shape");
        // the section holds everything its mode's layout addresses (the decoder trusts it)
        const int64_t np_ = n_pix[k], plane = np_ * n_obs[k], sec_bytes = off[k + 1] - off[k];
        const int32_t no_ = n_obs[k];
        const uint32_t *koff = reinterpret_cast<const uint32_t *>(ccd_enc_koff(sec));
        int rc;
        if (h->mode == CCD_ENC_MODE_RAW) {
            if (sec_bytes < ccd_enc_size_raw(plane)) return enc_fail(k, " raw section is truncated");
        } else if (h->mode == CCD_ENC_MODE_PACK) {
            // bit-packed runs: the kept table as in mode 1, then every run's descriptor against the
            // prefix sums of its code words (ceil(k w / 32)) and exceptions, the totals against the
            // header, and the section long enough for all five parts and the pad word -- after
            // this no code bit can send the decoder outside the section
            *packed = true;
            const int64_t kept = h->kept, code_words = h->code_words, exc_total = h->exc_total;
            if (kept < 0 || kept > plane || h->band_stride != 0 || code_words < 0 || exc_total < 0 ||
                code_words > 4 * plane + 8 * np_ || exc_total > 7 * plane ||
                sec_bytes < ccd_enc_size_pack_fixed(np_, no_))
                return enc_fail(k, " packed header does not fit its section");
            if ((rc = enc_check_koff(k, koff, np_, no_, kept))) return rc;
            const ccd_enc_run *runs = reinterpret_cast<const ccd_enc_run *>(ccd_enc_body(sec, np_, no_));
            int64_t cw = 0, ex = 0;
            for (int64_t r = 0; r < CCD_ENC_BANDS * np_; ++r) {
                const ccd_enc_run &d = runs[r];
                const int64_t kk = (int64_t)(koff[r / CCD_ENC_BANDS + 1] - koff[r / CCD_ENC_BANDS]);
                if (d.w > 16) return enc_fail(k, " run " + std::to_string(r) + " has a width above 16");
                if ((int64_t)d.code_word != cw || (int64_t)d.exc_off != ex)
                    return enc_fail(k, " run " + std::to_string(r) + " does not start at the prefix sums");
                if ((int64_t)d.n_exc > kk)
                    return enc_fail(k, " run " + std::to_string(r) + " has more exceptions than values");
                cw += (kk * d.w + 31) / 32;
                ex += d.n_exc;
            }
            if (cw != code_words || ex != exc_total)
                return enc_fail(k, " run totals do not match code_words / exc_total");
            if (sec_bytes < ccd_enc_size_pack(np_, no_, code_words, exc_total))
                return enc_fail(k, " packed section is truncated");
        } else {
            mode1 = true;
            const int64_t kept = h->kept, bstride = h->band_stride;
            if (kept < 0 || kept > plane || bstride < kept || bstride % 8 != 0 ||
                sec_bytes < ccd_enc_size_cols(np_, no_, bstride))
                return enc_fail(k, " band columns do not fit its section");
            if ((rc = enc_check_koff(k, koff, np_, no_, kept))) return rc;
        }
        pb += n_pix[k];
        db += (int64_t)n_pix[k] * n_obs[k];
    }
    if (pixo[n_chips] != pb) return fail(CCDGPU_EINVAL, "encoded batch: pixel total does not match");
    if (mode1 && *packed) return fail(CCDGPU_EINVAL, "encoded batch: mode 1 and mode 2 sections in one batch");
    return 0;
}

// Children have larger indices than their parents, so one pass in index order carries the depth
// down from the roots.
int forest_validate(const ccdgpu_forest *f, int32_t *max_depth) {
    if (!f) return fail(CCDGPU_EINVAL, "forest is NULL");
    if (f->n_trees < 1) return fail(CCDGPU_EINVAL, "forest: n_trees must be >= 1, got " + std::to_string(f->n_trees));
    if (f->n_nodes < 1) return fail(CCDGPU_EINVAL, "forest: n_nodes must be >= 1, got " + std::to_string(f->n_nodes));
    if (f->n_features < 1 || f->n_features > CCDGPU_FOREST_MAX_FEATURES)
        return fail(CCDGPU_EINVAL, "forest: n_features must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_FEATURES) + "], got " +
                                       std::to_string(f->n_features));
    if (f->n_classes < 1 || f->n_classes > CCDGPU_FOREST_MAX_CLASSES)
        return fail(CCDGPU_EINVAL, "forest: n_classes must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_CLASSES) + "], got " +
                                       std::to_string(f->n_classes));
    if (!f->root || !f->feature || !f->threshold || !f->left || !f->right || !f->value)
        return fail(CCDGPU_EINVAL, "forest: NULL array");
    const int32_t nn = f->n_nodes, nc = f->n_classes;
    // depth of a node below its root; -1: not reached from any root; parents counted in `seen`
    std::vector<int32_t> depth((size_t)nn, -1);
    std::vector<unsigned char> seen((size_t)nn, 0);
    for (int32_t t = 0; t < f->n_trees; ++t) {
        const int32_t r = f->root[t];
        if (r < 0 || r >= nn)
            return fail(CCDGPU_EINVAL, "forest: root of tree " + std::to_string(t) + " is " + std::to_string(r) +
                                           ", outside [0, " + std::to_string(nn) + ")");
        if (seen[r]) return fail(CCDGPU_EINVAL, "forest: node " + std::to_string(r) + " is the root of two trees (shared node)");
        seen[r] = 1;
        depth[r] = 0;
    }
    int32_t deepest = 0;
    for (int32_t n = 0; n < nn; ++n) {
        if (f->feature[n] < 0) {
            for (int32_t k = 0; k < nc; ++k)
                if (!std::isfinite(f->value[(size_t)n * nc + k]))
                    return fail(CCDGPU_EINVAL, "forest: leaf " + std::to_string(n) + " has a non-finite value (class " +
                                                   std::to_string(k) + ")");
            if (depth[n] > deepest) deepest = depth[n];
            continue;
        }
        if (f->feature[n] >= f->n_features)
            return fail(CCDGPU_EINVAL, "forest: node " + std::to_string(n) + " tests feature " + std::to_string(f->feature[n]) +
                                           " >= n_features " + std::to_string(f->n_features));
        if (!std::isfinite(f->threshold[n]))
            return fail(CCDGPU_EINVAL, "forest: node " + std::to_string(n) + " has a non-finite threshold");
        const int32_t ch[2] = {f->left[n], f->right[n]};
        for (int32_t side = 0; side < 2; ++side) {
            const int32_t c = ch[side];
            const char *name = side ? "right" : "left";
            if (c < 0 || c >= nn)
                return fail(CCDGPU_EINVAL, "forest: " + std::string(name) + " child of node " + std::to_string(n) + " is " +
                                               std::to_string(c) + ", outside [0, " + std::to_string(nn) + ")");
            if (c <= n)
                return fail(CCDGPU_EINVAL, "forest: " + std::string(name) + " child of node " + std::to_string(n) + " is " +
                                               std::to_string(c) + ", not greater than its parent's index");
            if (seen[c]) return fail(CCDGPU_EINVAL, "forest: node " + std::to_string(c) + " has two parents (shared node)");
            seen[c] = 1;
            if (depth[n] >= 0) depth[c] = depth[n] + 1;
        }
    }
    if (max_depth) *max_depth = deepest;
    return 0;
}

int forest_build(const ccdgpu_forest *f, int32_t cap, std::vector<unsigned char> &pool, std::vector<int64_t> &tree_off,
                 std::vector<int32_t> &chunk_first) {
    const int32_t nt = f->n_trees, nc = f->n_classes;
    tree_off.assign((size_t)nt + 1, 0);
    pool.clear();
    std::vector<int32_t> order;
    for (int32_t t = 0; t < nt; ++t) {
        order.assign(1, f->root[t]);
        size_t leaves = 0;
        for (size_t i = 0; i < order.size(); ++i) {
            const int32_t n = order[i];
            if (f->feature[n] < 0) {
                ++leaves;
            } else {
                order.push_back(f->left[n]);
                order.push_back(f->right[n]);
            }
        }
        const size_t n_t = order.size();
        const size_t bytes = (n_t * sizeof(CcdForestNode) + leaves * nc * sizeof(double) + 15) & ~(size_t)15;
        if (bytes / 8 >= (size_t)INT32_MAX) return fail(CCDGPU_EINVAL, "forest: tree " + std::to_string(t) + " is too large");
        const size_t at = pool.size();
        pool.resize(at + bytes, 0);
        CcdForestNode *nodes = reinterpret_cast<CcdForestNode *>(pool.data() + at);
        double *vals = reinterpret_cast<double *>(pool.data() + at);
        size_t next = 1, leaf = 0;
        for (size_t i = 0; i < n_t; ++i) {
            const int32_t n = order[i];
            if (f->feature[n] < 0) {
                const size_t v = n_t * sizeof(CcdForestNode) / sizeof(double) + leaf * nc;
                nodes[i].threshold = 0.0;
                nodes[i].feature = -1;
                nodes[i].left = (int32_t)v;
                std::memcpy(vals + v, f->value + (size_t)n * nc, sizeof(double) * nc);
                ++leaf;
            } else {
                nodes[i].threshold = f->threshold[n];
                nodes[i].feature = f->feature[n];
                nodes[i].left = (int32_t)next;
                next += 2;
            }
        }
        tree_off[t + 1] = (int64_t)pool.size();
    }
    chunk_first.assign(1, 0);
    for (int32_t t = 0; t < nt;) {
        int32_t e = t + 1;
        if (tree_off[e] - tree_off[t] <= cap)
            while (e < nt && tree_off[e + 1] - tree_off[t] <= cap) ++e;
        chunk_first.push_back(e);
        t = e;
    }
    return 0;
}

// the date vector of a prediction or product request (`who`: "predict" / "products")
static int check_dates(const std::string &who, int64_t n_dates, const int64_t *dates) {
    if (n_dates < 0) return fail(CCDGPU_EINVAL, who + ": n_dates must be >= 0, got " + std::to_string(n_dates));
    if (n_dates > INT32_MAX) return fail(CCDGPU_EINVAL, who + ": n_dates must be < 2^31, got " + std::to_string(n_dates));
    if (n_dates > 0 && !dates) return fail(CCDGPU_EINVAL, who + ": dates is NULL");
    for (int64_t i = 0; i < n_dates; ++i)
        if (dates[i] < 1 || dates[i] > CCDGPU_PREDICT_MAX_DATE)
            return fail(CCDGPU_EINVAL, who + ": dates[" + std::to_string(i) + "] = " + std::to_string(dates[i]) +
                                           " is outside 1 .. " + std::to_string(CCDGPU_PREDICT_MAX_DATE));
    return 0;
}

// the row table of a prediction or product request: counts, pointers, offsets
static int check_table(const std::string &who, int64_t n_pix, const int64_t *row_offsets, int64_t n_rows, const ccdgpu_row *rows) {
    if (n_pix < 0) return fail(CCDGPU_EINVAL, who + ": n_pix must be >= 0, got " + std::to_string(n_pix));
    if (n_rows < 0) return fail(CCDGPU_EINVAL, who + ": n_rows must be >= 0, got " + std::to_string(n_rows));
    if (!row_offsets) return fail(CCDGPU_EINVAL, who + ": row_offsets is NULL");
    if (n_rows > 0 && !rows) return fail(CCDGPU_EINVAL, who + ": rows is NULL");
    if (row_offsets[0] != 0)
        return fail(CCDGPU_EINVAL, who + ": row_offsets[0] must be 0, got " + std::to_string(row_offsets[0]));
    for (int64_t p = 0; p < n_pix; ++p)
        if (row_offsets[p + 1] < row_offsets[p])
            return fail(CCDGPU_EINVAL, who + ": row_offsets decrease at pixel " + std::to_string(p) + " (" +
                                           std::to_string(row_offsets[p]) + " -> " + std::to_string(row_offsets[p + 1]) + ")");
    if (row_offsets[n_pix] != n_rows)
        return fail(CCDGPU_EINVAL, who + ": row_offsets[n_pix] is " + std::to_string(row_offsets[n_pix]) + ", n_rows is " +
                                       std::to_string(n_rows));
    return 0;
}

int predict_check_dates(int64_t n_dates, const int64_t *dates, double avg_days_yr) {
    // (a bad count or pointer is named before avg_days_yr, a bad date after it)
    if (n_dates < 0 || n_dates > INT32_MAX || (n_dates > 0 && !dates)) return check_dates("predict", n_dates, dates);
    if (!std::isfinite(avg_days_yr) || !(avg_days_yr > 0.0))
        return fail(CCDGPU_EINVAL, "predict: avg_days_yr must be finite and > 0, got " + std::to_string(avg_days_yr));
    return check_dates("predict", n_dates, dates);
}

int predict_check_modes(int32_t cover, int32_t dtype) {
    if (cover != CCDGPU_COVER_SPAN && cover != CCDGPU_COVER_EXTEND)
        return fail(CCDGPU_EINVAL, "predict: unknown cover " + std::to_string(cover));
    if (dtype != CCDGPU_PREDICT_F32 && dtype != CCDGPU_PREDICT_I16)
        return fail(CCDGPU_EINVAL, "predict: unknown dtype " + std::to_string(dtype));
    return 0;
}

// 1 January of proleptic-Gregorian year y as an ordinal (y >= 1)
static int64_t year_start(int64_t y) {
    const int64_t p = y - 1;
    return p * 365 + p / 4 - p / 100 + p / 400 + 1;
}

void year_window(int64_t t, int64_t *a, int64_t *b) {
    // the year of ordinal t: 400-, 100-, 4- and 1-year cycles of 146097, 36524, 1461 and 365 days
    int64_t n = t - 1;
    const int64_t n400 = n / 146097;
    n %= 146097;
    const int64_t n100 = n / 36524;
    n %= 36524;
    const int64_t n4 = n / 1461;
    n %= 1461;
    const int64_t n1 = n / 365;
    int64_t y = n400 * 400 + n100 * 100 + n4 * 4 + n1 + 1;
    if (n1 == 4 || n100 == 4) --y;  // 31 December of a leap year
    *a = year_start(y);
    *b = year_start(y + 1);
}

int products_check_params(const ccdgpu_product_params *p, const float *rfrawp, const struct ccdgpu_products *out) {
    if (!p) return fail(CCDGPU_EINVAL, "products: params is NULL");
    if (!out) return fail(CCDGPU_EINVAL, "products: out is NULL");
    if (p->bot < 1 || p->bot > CCDGPU_PREDICT_MAX_DATE)
        return fail(CCDGPU_EINVAL, "products: bot = " + std::to_string(p->bot) + " is outside 1 .. " +
                                       std::to_string(CCDGPU_PREDICT_MAX_DATE));
    if (p->mag_bands & ~0x7Fu) return fail(CCDGPU_EINVAL, "products: mag_bands must only use bits 0..6");
    if (p->n_classes < 0 || p->n_classes > 32)
        return fail(CCDGPU_EINVAL, "products: n_classes must be in [0, 32], got " + std::to_string(p->n_classes));
    for (int32_t k = 0; k < p->n_classes; ++k)
        if (p->labels[k] == 0) return fail(CCDGPU_EINVAL, "products: labels[" + std::to_string(k) + "] is 0 (labels are 1 .. 255)");
    if (p->cover != CCDGPU_COVER_SPAN && p->cover != CCDGPU_COVER_EXTEND)
        return fail(CCDGPU_EINVAL, "products: unknown cover " + std::to_string(p->cover));
    const bool cover_out = out->lcpri || out->lcsec || out->lcpconf || out->lcsconf || out->lcachg;
    if (cover_out && !rfrawp) return fail(CCDGPU_EINVAL, "products: a cover product is requested but rfrawp is NULL");
    if (cover_out && p->n_classes == 0) return fail(CCDGPU_EINVAL, "products: a cover product is requested but n_classes is 0");
    if (!cover_out && !out->sctime && !out->scmag && !out->sclast && !out->scstab && !out->scmqa)
        return fail(CCDGPU_EINVAL, "products: no product is requested (all ten outputs are NULL)");
    return 0;
}

int products_check_dates(int64_t n_dates, const int64_t *dates) { return check_dates("products", n_dates, dates); }

int train_validate(const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features, int32_t n_classes,
                   const double *edges, const int32_t *n_edges, const ccdgpu_train_params *p) {
    const std::string who = "train: ";
    if (!p) return fail(CCDGPU_EINVAL, who + "params is NULL");
    if (!x) return fail(CCDGPU_EINVAL, who + "x is NULL");
    if (!labels) return fail(CCDGPU_EINVAL, who + "labels is NULL");
    if (!n_edges) return fail(CCDGPU_EINVAL, who + "n_edges is NULL");
    if (n_rows < 1 || n_rows > CCDGPU_TRAIN_MAX_ROWS)
        return fail(CCDGPU_EINVAL, who + "n_rows must be in [1, 2^27], got " + std::to_string(n_rows));
    if (n_features < 1 || n_features > CCDGPU_FOREST_MAX_FEATURES)
        return fail(CCDGPU_EINVAL, who + "n_features must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_FEATURES) + "], got " +
                                       std::to_string(n_features));
    if (n_classes < 1 || n_classes > CCDGPU_FOREST_MAX_CLASSES)
        return fail(CCDGPU_EINVAL, who + "n_classes must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_CLASSES) + "], got " +
                                       std::to_string(n_classes));
    if (p->max_depth < 0 || p->max_depth > CCDGPU_TRAIN_MAX_DEPTH)
        return fail(CCDGPU_EINVAL, who + "max_depth must be in [0, " + std::to_string(CCDGPU_TRAIN_MAX_DEPTH) + "], got " +
                                       std::to_string(p->max_depth));
    if (p->n_trees < 1 || p->n_trees > INT32_MAX / ((2 << p->max_depth) - 1))
        return fail(CCDGPU_EINVAL, who + "n_trees must be in [1, " + std::to_string(INT32_MAX / ((2 << p->max_depth) - 1)) +
                                       "] at max_depth " + std::to_string(p->max_depth) + ", got " + std::to_string(p->n_trees));
    if (p->features_per_node < 0)
        return fail(CCDGPU_EINVAL, who + "features_per_node must be >= 0, got " + std::to_string(p->features_per_node));
    if (p->min_instances_per_node < 1)
        return fail(CCDGPU_EINVAL, who + "min_instances_per_node must be >= 1, got " + std::to_string(p->min_instances_per_node));
    if (!std::isfinite(p->min_info_gain) || p->min_info_gain < 0.0)
        return fail(CCDGPU_EINVAL, who + "min_info_gain must be finite and >= 0, got " + std::to_string(p->min_info_gain));
    if (p->bootstrap != 0 && p->bootstrap != 1)
        return fail(CCDGPU_EINVAL, who + "bootstrap must be 0 or 1, got " + std::to_string(p->bootstrap));
    int64_t total_edges = 0;
    for (int32_t f = 0; f < n_features; ++f) {
        if (n_edges[f] < 0 || n_edges[f] > CCDGPU_TRAIN_MAX_EDGES)
            return fail(CCDGPU_EINVAL, who + "n_edges[" + std::to_string(f) + "] must be in [0, " +
                                           std::to_string(CCDGPU_TRAIN_MAX_EDGES) + "], got " + std::to_string(n_edges[f]));
        total_edges += n_edges[f];
    }
    if (total_edges > 0 && !edges) return fail(CCDGPU_EINVAL, who + "edges is NULL");
    for (int32_t f = 0, at = 0; f < n_features; at += n_edges[f], ++f)
        for (int32_t b = 0; b < n_edges[f]; ++b) {
            if (!std::isfinite(edges[at + b]))
                return fail(CCDGPU_EINVAL, who + "edges of feature " + std::to_string(f) + ": edge " + std::to_string(b) +
                                               " is not finite");
            if (b > 0 && !(edges[at + b] > edges[at + b - 1]))
                return fail(CCDGPU_EINVAL, who + "edges of feature " + std::to_string(f) + ": edge " + std::to_string(b) +
                                               " is not above edge " + std::to_string(b - 1));
        }
    for (int64_t r = 0; r < n_rows; ++r)
        if (labels[r] < 0 || labels[r] >= n_classes)
            return fail(CCDGPU_EINVAL, who + "labels[" + std::to_string(r) + "] = " + std::to_string(labels[r]) +
                                           " is outside 0 .. " + std::to_string(n_classes - 1));
    for (int64_t i = 0, n = n_rows * n_features; i < n; ++i)
        if (!std::isfinite(x[i]))
            return fail(CCDGPU_EINVAL, who + "x[" + std::to_string(i / n_features) + "][" + std::to_string(i % n_features) +
                                           "] is not finite");
    return 0;
}

int32_t train_features_per_node(int32_t n_features, const ccdgpu_train_params *p) {
    int32_t m = p->features_per_node;
    if (m == 0)
        while (m * m < n_features) ++m;
    return m < n_features ? m : n_features;
}

int splits_validate(const double *x, int64_t n_rows, int32_t n_features, int32_t max_bins) {
    const std::string who = "splits: ";
    if (n_rows < 0 || n_rows > CCDGPU_TRAIN_MAX_ROWS)
        return fail(CCDGPU_EINVAL, who + "n_rows must be in [0, 2^27], got " + std::to_string(n_rows));
    if (n_features < 1 || n_features > CCDGPU_FOREST_MAX_FEATURES)
        return fail(CCDGPU_EINVAL, who + "n_features must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_FEATURES) + "], got " +
                                       std::to_string(n_features));
    if (max_bins < 2 || max_bins > CCDGPU_TRAIN_MAX_EDGES + 1)
        return fail(CCDGPU_EINVAL, who + "max_bins must be in [2, " + std::to_string(CCDGPU_TRAIN_MAX_EDGES + 1) + "], got " +
                                       std::to_string(max_bins));
    if (n_rows == 0) return 0;
    if (!x) return fail(CCDGPU_EINVAL, who + "x is NULL");
    for (int64_t i = 0, n = n_rows * n_features; i < n; ++i)
        if (!std::isfinite(x[i]))
            return fail(CCDGPU_EINVAL, who + "x[" + std::to_string(i / n_features) + "][" + std::to_string(i % n_features) +
                                           "] is not finite");
    return 0;
}

int oob_validate(const double *x, int64_t n_rows, const ccdgpu_oob_params *p, const float *oob_raw, const int32_t *n_oob) {
    const std::string who = "oob: ";
    if (!p) return fail(CCDGPU_EINVAL, who + "params is NULL");
    if (n_rows < 0 || n_rows > CCDGPU_TRAIN_MAX_ROWS)
        return fail(CCDGPU_EINVAL, who + "n_rows must be in [0, 2^27], got " + std::to_string(n_rows));
    if (p->first_row < 0 || p->first_row > CCDGPU_TRAIN_MAX_ROWS - n_rows)
        return fail(CCDGPU_EINVAL, who + "first_row must be in [0, 2^27 - n_rows], got " + std::to_string(p->first_row) +
                                       " with " + std::to_string(n_rows) + " rows");
    if (n_rows == 0) return 0;
    if (!x) return fail(CCDGPU_EINVAL, who + "x is NULL");
    if (!oob_raw) return fail(CCDGPU_EINVAL, who + "oob_raw is NULL");
    if (!n_oob) return fail(CCDGPU_EINVAL, who + "n_oob is NULL");
    return 0;
}

int permutation_validate(const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features, int32_t n_classes,
                         const ccdgpu_permutation_params *p, const int64_t *oob_rows, const int64_t *correct, const int64_t *lost,
                         const int64_t *gained) {
    const std::string who = "permutation: ";
    if (!p) return fail(CCDGPU_EINVAL, who + "params is NULL");
    if (!oob_rows) return fail(CCDGPU_EINVAL, who + "oob_rows is NULL");
    if (!correct) return fail(CCDGPU_EINVAL, who + "correct is NULL");
    if (!lost) return fail(CCDGPU_EINVAL, who + "lost is NULL");
    if (!gained) return fail(CCDGPU_EINVAL, who + "gained is NULL");
    if (n_rows < 0 || n_rows > CCDGPU_TRAIN_MAX_ROWS)
        return fail(CCDGPU_EINVAL, who + "n_rows must be in [0, 2^27], got " + std::to_string(n_rows));
    if (n_features < 1 || n_features > CCDGPU_FOREST_MAX_FEATURES)
        return fail(CCDGPU_EINVAL, who + "n_features must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_FEATURES) + "], got " +
                                       std::to_string(n_features));
    if (n_classes < 1 || n_classes > CCDGPU_FOREST_MAX_CLASSES)
        return fail(CCDGPU_EINVAL, who + "n_classes must be in [1, " + std::to_string(CCDGPU_FOREST_MAX_CLASSES) + "], got " +
                                       std::to_string(n_classes));
    if (n_rows == 0) return 0;
    if (!x) return fail(CCDGPU_EINVAL, who + "x is NULL");
    if (!labels) return fail(CCDGPU_EINVAL, who + "labels is NULL");
    for (int64_t r = 0; r < n_rows; ++r)
        if (labels[r] < 0 || labels[r] >= n_classes)
            return fail(CCDGPU_EINVAL, who + "labels[" + std::to_string(r) + "] = " + std::to_string(labels[r]) +
                                           " is outside 0 .. " + std::to_string(n_classes - 1));
    return 0;
}

}  // namespace ccdhost

using namespace ccdhost;

extern "C" {

const char *ccdgpu_last_error(void) { return g_err.c_str(); }

void ccdgpu_params_default(ccdgpu_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->meow_size = 12;
    p->peek_size = 6;
    p->day_delta = 365;
    p->coef_min = 4;
    p->coef_mid = 6;
    p->coef_max = 8;
    p->num_obs_factor = 3;
    p->detection_bands = 0x3E;
    p->tmask_bands = 0x12;
    p->lasso_max_iter = 1000;
    p->thermal_min = -9320;
    p->thermal_max = 7070;
    p->median_green_filter = 400;
    p->curve_qa_start = 14;
    p->curve_qa_end = 24;
    p->curve_qa_insuf_clear = 44;
    p->curve_qa_persist_snow = 54;
    p->qa_fill = 0;
    p->qa_clear = 1;
    p->qa_water = 2;
    p->qa_shadow = 3;
    p->qa_snow = 4;
    p->qa_cloud = 5;
    p->qa_cirrus1 = 8;
    p->qa_cirrus2 = 9;
    p->qa_occlusion = 10;
    p->qa_bitpacked = 1;
    p->adaptive_peek = 1;
    p->rmse_dof = 0;
    p->kelvin_to_celsius = 1;
    p->avg_days_yr = 365.2425;
    p->change_probability = 0.99;
    p->change_threshold = 15.086272469388987;
    p->outlier_threshold = 35.888186879610423;
    p->t_const = 4.42;
    p->lasso_alpha = 1.0;
    p->lasso_tol = 1e-4;
    p->clear_pct_threshold = 0.25;
    p->snow_pct_threshold = 0.75;
    p->argsort_stable = 0;  // numpy quicksort tie order (include/ccdgpu.h)
    p->reserved0 = 0;
}

int ccdgpu_encoded_check(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, const uint8_t *enc,
                         int64_t enc_bytes) {
    bool packed;
    return encoded_check(n_chips, n_pix, n_obs, enc, enc_bytes, &packed);
}

int ccdgpu_forest_check(const ccdgpu_forest *f) { return forest_validate(f, nullptr); }

int ccdgpu_forest_depth(const ccdgpu_forest *f, int32_t *max_depth) {
    if (!max_depth) return fail(CCDGPU_EINVAL, "NULL argument");
    *max_depth = 0;
    return forest_validate(f, max_depth);
}

void ccdgpu_train_params_default(ccdgpu_train_params *p) {
    if (!p) return;
    *p = ccdgpu_train_params{};
    p->n_trees = 500;
    p->max_depth = 5;
    p->min_instances_per_node = 1;
    p->bootstrap = 1;
}

int ccdgpu_train_check(const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features, int32_t n_classes,
                       const double *edges, const int32_t *n_edges, const ccdgpu_train_params *params) {
    return train_validate(x, labels, n_rows, n_features, n_classes, edges, n_edges, params);
}

int ccdgpu_splits_check(const double *x, int64_t n_rows, int32_t n_features, int32_t max_bins) {
    return splits_validate(x, n_rows, n_features, max_bins);
}

int ccdgpu_oob_check(const double *x, int64_t n_rows, const ccdgpu_oob_params *params, const float *oob_raw,
                     const int32_t *n_oob) {
    return oob_validate(x, n_rows, params, oob_raw, n_oob);
}

int ccdgpu_permutation_check(const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features, int32_t n_classes,
                             const ccdgpu_permutation_params *params, const int64_t *oob_rows, const int64_t *correct,
                             const int64_t *lost, const int64_t *gained) {
    return permutation_validate(x, labels, n_rows, n_features, n_classes, params, oob_rows, correct, lost, gained);
}

int ccdgpu_predict_check(int64_t n_pix, const int64_t *row_offsets, int64_t n_rows, const ccdgpu_row *rows, int64_t n_dates,
                         const int64_t *dates, double avg_days_yr, int32_t cover, int32_t dtype) {
    int rc = check_table("predict", n_pix, row_offsets, n_rows, rows);
    if (rc || (rc = predict_check_dates(n_dates, dates, avg_days_yr))) return rc;
    return predict_check_modes(cover, dtype);
}

void ccdgpu_product_params_default(ccdgpu_product_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->bot = 723546;  // 1982-01-01
    p->mag_bands = 0x3E;
    p->cover = CCDGPU_COVER_EXTEND;
    p->n_classes = 0;
    for (int k = 0; k < 32; ++k) p->labels[k] = (uint8_t)(k + 1);
}

int ccdgpu_year_window(int64_t t, int64_t *a, int64_t *b) {
    if (!a || !b) return fail(CCDGPU_EINVAL, "year_window: NULL argument");
    if (t < 1 || t > CCDGPU_PREDICT_MAX_DATE)
        return fail(CCDGPU_EINVAL, "year_window: t = " + std::to_string(t) + " is outside 1 .. " +
                                       std::to_string(CCDGPU_PREDICT_MAX_DATE));
    year_window(t, a, b);
    return 0;
}

int ccdgpu_products_check(int64_t n_pix, const int64_t *row_offsets, int64_t n_rows, const ccdgpu_row *rows, const float *rfrawp,
                          int64_t n_dates, const int64_t *dates, const ccdgpu_product_params *params,
                          const struct ccdgpu_products *out) {
    int rc = check_table("products", n_pix, row_offsets, n_rows, rows);
    if (rc || (rc = products_check_dates(n_dates, dates))) return rc;
    return products_check_params(params, rfrawp, out);
}

}  // extern "C"
