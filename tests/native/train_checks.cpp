/* CPU check of the training request's validator (lcmap-firebird_amd/csrc/ccdgpu_checks.cpp): a
 * stand-alone program, built with -fsanitize=address,undefined and run by
 * tests/test_randomforest_train.py.  ccdgpu_train_check on rows, labels, edges and edge counts given
 * in heap blocks of exactly their size, so a read past them is a sanitizer error: the accepted edge
 * cases and every rejection. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../include/ccdgpu.h"

#define REQUIRE(cond, what)                                                                 \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::printf("%s:%d: %s (%s) -- %s\n", __FILE__, __LINE__, what, #cond, ccdgpu_last_error()); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

static bool refused(int rc, const char *needle) { return rc == CCDGPU_EINVAL && std::strstr(ccdgpu_last_error(), needle); }

static int checks() {
    // 5 rows of 3 features with 2, 0 and 1 edges; everything in heap blocks of exactly its size
    const int64_t n_rows = 5;
    const int32_t nf = 3, nc = 4;
    double *x = (double *)std::malloc(sizeof(double) * n_rows * nf);
    int32_t *y = (int32_t *)std::malloc(sizeof(int32_t) * n_rows);
    double *edges = (double *)std::malloc(sizeof(double) * 3);
    int32_t *ne = (int32_t *)std::malloc(sizeof(int32_t) * nf);
    ccdgpu_train_params *p = (ccdgpu_train_params *)std::malloc(sizeof(ccdgpu_train_params));
    for (int64_t i = 0; i < n_rows * nf; ++i) x[i] = (double)i * 0.5;
    for (int64_t r = 0; r < n_rows; ++r) y[r] = (int32_t)(r % nc);
    edges[0] = -1.0, edges[1] = 2.0, edges[2] = 0.0;
    ne[0] = 2, ne[1] = 0, ne[2] = 1;
    ccdgpu_train_params_default(p);
    REQUIRE(p->n_trees == 500 && p->max_depth == 5 && p->features_per_node == 0 && p->min_instances_per_node == 1 &&
                p->min_info_gain == 0.0 && p->bootstrap == 1 && p->seed == 0,
            "default parameters");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    REQUIRE(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p) == 0, "a good request");
    REQUIRE(ccdgpu_train_check(x, y, 1, nf, nc, edges, ne, p) == 0, "one row");
    p->max_depth = 0;
    p->bootstrap = 0;
    p->features_per_node = 1000;
    p->seed = ~(uint64_t)0;
    REQUIRE(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p) == 0, "depth 0, no bootstrap, a clamped subset size");
    ccdgpu_train_params_default(p);
    ne[0] = 0, ne[2] = 0;
    REQUIRE(ccdgpu_train_check(x, y, n_rows, nf, nc, nullptr, ne, p) == 0, "no edges at all: edges may be NULL");
    ne[0] = 2, ne[2] = 1;
    // NULLs
    REQUIRE(refused(ccdgpu_train_check(nullptr, y, n_rows, nf, nc, edges, ne, p), "x is NULL"), "NULL x");
    REQUIRE(refused(ccdgpu_train_check(x, nullptr, n_rows, nf, nc, edges, ne, p), "labels is NULL"), "NULL labels");
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, nullptr, ne, p), "edges is NULL"), "NULL edges");
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, nullptr, p), "n_edges is NULL"), "NULL n_edges");
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, nullptr), "params is NULL"), "NULL params");
    // counts (refused before any array is read: the blocks are too small for these sizes)
    REQUIRE(refused(ccdgpu_train_check(x, y, 0, nf, nc, edges, ne, p), "n_rows"), "no rows");
    REQUIRE(refused(ccdgpu_train_check(x, y, CCDGPU_TRAIN_MAX_ROWS + 1, nf, nc, edges, ne, p), "n_rows"), "too many rows");
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, 0, nc, edges, ne, p), "n_features"), "no features");
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, CCDGPU_FOREST_MAX_FEATURES + 1, nc, edges, ne, p), "n_features"), "65 features");
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, 0, edges, ne, p), "n_classes"), "no classes");
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, CCDGPU_FOREST_MAX_CLASSES + 1, edges, ne, p), "n_classes"), "33 classes");
    // edges
    ne[1] = CCDGPU_TRAIN_MAX_EDGES + 1;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "n_edges[1]"), "64 edges");
    ne[1] = -1;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "n_edges[1]"), "negative edge count");
    ne[1] = 0;
    edges[1] = -1.0;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "feature 0: edge 1 is not above"), "equal edges");
    edges[1] = -2.0;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "feature 0: edge 1 is not above"), "decreasing edges");
    edges[1] = inf;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "feature 0: edge 1 is not finite"), "infinite edge");
    edges[1] = 2.0;
    edges[2] = nan;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "feature 2: edge 0 is not finite"), "NaN edge");
    edges[2] = 0.0;
    // labels and rows: the last element of each block
    y[n_rows - 1] = nc;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "labels[4] = 4"), "label past the classes");
    y[n_rows - 1] = -1;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "labels[4] = -1"), "negative label");
    y[n_rows - 1] = nc - 1;
    REQUIRE(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p) == 0, "the last class is a label");
    x[n_rows * nf - 1] = nan;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "x[4][2] is not finite"), "NaN value");
    x[n_rows * nf - 1] = -inf;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "x[4][2] is not finite"), "infinite value");
    x[n_rows * nf - 1] = 1e300;
    REQUIRE(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p) == 0, "a large finite value");
    // parameters
    p->n_trees = 0;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "n_trees"), "no trees");
    p->n_trees = INT32_MAX;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "n_trees"), "more nodes than int32 holds");
    p->max_depth = 0;
    REQUIRE(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p) == 0, "2^31 - 1 single-leaf trees");
    ccdgpu_train_params_default(p);
    p->max_depth = -1;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "max_depth"), "negative depth");
    p->max_depth = CCDGPU_TRAIN_MAX_DEPTH + 1;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "max_depth"), "depth 11");
    p->max_depth = CCDGPU_TRAIN_MAX_DEPTH;
    REQUIRE(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p) == 0, "depth 10");
    p->features_per_node = -1;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "features_per_node"), "negative subset size");
    p->features_per_node = 0;
    p->min_instances_per_node = 0;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "min_instances_per_node"), "no instances");
    p->min_instances_per_node = 1;
    p->min_info_gain = -1e-9;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "min_info_gain"), "negative gain");
    p->min_info_gain = nan;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "min_info_gain"), "NaN gain");
    p->min_info_gain = 0.0;
    p->bootstrap = 2;
    REQUIRE(refused(ccdgpu_train_check(x, y, n_rows, nf, nc, edges, ne, p), "bootstrap"), "bootstrap 2");
    std::free(x);
    std::free(y);
    std::free(edges);
    std::free(ne);
    std::free(p);
    return 0;
}

int main() {
    if (checks()) return 1;
    std::printf("ok\n");
    return 0;
}
