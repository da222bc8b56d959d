// ccdgpu_checks.h -- the host API's error state and the validators of everything a caller hands
// over (ccdgpu_checks.cpp).  No HIP: this much of the host side also builds with a plain C++
// compiler, so the checks can run in a stand-alone program under sanitizers
// (tests/native/host_checks.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ccdgpu.h"
#include "ccd_device.h"

namespace ccdhost {

// records msg as the calling thread's ccdgpu_last_error and returns code
int fail(int code, const std::string &msg);

// Shape of a staged batch: per-chip pixel / observation counts and their prefix sums
// (ccd_device.h layout).
struct Shape {
    std::vector<int32_t> npix, nobs;
    std::vector<int64_t> obs_off, pix_off, data_off;  // [n_chips + 1]
    int32_t n_obs_max = 0;
    int n_chips() const { return (int)npix.size(); }
    int64_t total_obs() const { return obs_off.empty() ? 0 : obs_off.back(); }
    int64_t total_pix() const { return pix_off.empty() ? 0 : pix_off.back(); }
    int64_t total_data() const { return data_off.empty() ? 0 : data_off.back(); }
};

int make_shape(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, Shape &s);
int check_params(const ccdgpu_params *p);
// change threshold per (adaptive) peek size: CcdDetectArgs::thr_table [CCDGPU_MAX_PEEK + 1]
void fill_thr_table(const ccdgpu_params &p, double *thr);

// ccdgpu_encoded_check (layout: ccd_enc_layout.h); *packed: the batch holds a mode 2 section (it
// goes to ccd_decode_pack)
int encoded_check(int32_t n_chips, const int32_t *n_pix, const int32_t *n_obs, const uint8_t *enc, int64_t enc_bytes,
                  bool *packed);

// The checks of ccdgpu_forest_check, and the forest's depth (branches from a root to its deepest
// leaf).
int forest_validate(const ccdgpu_forest *f, int32_t *max_depth);
// The device form of a checked forest (ccd_device.h): per tree one blob, nodes breadth-first so
// that the children of a node are adjacent, the leaves' class vectors behind the nodes; then the
// chunks: runs of whole trees that fit `cap` bytes, a larger tree alone.
int forest_build(const ccdgpu_forest *f, int32_t cap, std::vector<unsigned char> &pool, std::vector<int64_t> &tree_off,
                 std::vector<int32_t> &chunk_first);

// The checks of ccdgpu_train_check, and the m of the rule's feature subsets (features_per_node with
// 0 resolved to the smallest m with m * m >= n_features, clamped to n_features).
int train_validate(const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features, int32_t n_classes,
                   const double *edges, const int32_t *n_edges, const ccdgpu_train_params *p);
int32_t train_features_per_node(int32_t n_features, const ccdgpu_train_params *p);
// The checks of ccdgpu_splits_check.
int splits_validate(const double *x, int64_t n_rows, int32_t n_features, int32_t max_bins);
// The checks of ccdgpu_oob_check.
int oob_validate(const double *x, int64_t n_rows, const ccdgpu_oob_params *p, const float *oob_raw, const int32_t *n_oob);
// The checks of ccdgpu_permutation_check.
int permutation_validate(const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features, int32_t n_classes,
                         const ccdgpu_permutation_params *p, const int64_t *oob_rows, const int64_t *correct, const int64_t *lost,
                         const int64_t *gained);

int predict_check_dates(int64_t n_dates, const int64_t *dates, double avg_days_yr);
int predict_check_modes(int32_t cover, int32_t dtype);

// a(t), b(t) of the product rule (include/ccdgpu.h) for a checked date t
void year_window(int64_t t, int64_t *a, int64_t *b);
// the parts of ccdgpu_products_check the chained path shares: the date vector; the parameters and outputs
int products_check_dates(int64_t n_dates, const int64_t *dates);
int products_check_params(const ccdgpu_product_params *p, const float *rfrawp, const struct ccdgpu_products *out);

}  // namespace ccdhost
