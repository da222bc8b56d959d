// ccdgpu_train.cpp -- training of the random forest on the device (include/ccdgpu.h states the rule;
// kernels in ccd_train.hip; the request's checks in ccdgpu_checks.cpp).
//
// The host drives the levels: per group of trees and level it names the level's open nodes and their
// feature subsets, launches the histogram and split kernels, reads back each node's class counts and
// chosen split, decides from the counts which children are leaves (depth, purity, size) and which are
// the next level's nodes, and has the rows moved there.  When a group is done its trees are written
// out in pre-order.  Only nodes that can still split are ever on the device, so a level's histograms
// are bounded by min(2^(max_depth-1), n_rows) nodes per tree.
#include <algorithm>
#include <cstdlib>
#include <utility>

#include "ccd_train.h"
#include "ccdgpu_host.h"

using namespace ccdhost;

namespace {

// rows binned per upload of x
const int64_t TRAIN_SLAB_ROWS = (int64_t)1 << 20;
// device bytes a group of trees may take for its row assignments and histograms
const int64_t TRAIN_GROUP_BYTES = (int64_t)1 << 30;

struct Open {  // a node of the current level that may still split
    int32_t g;   // tree within the group
    int32_t id;  // node number in the tree (root 1, children 2i and 2i + 1)
};

// a group's trees while they grow: per tree, by node number, the split (feature < 0: a leaf,
// seen == 0: no such node) and the class counts
struct Grown {
    int32_t per_tree = 0, n_classes = 0;
    std::vector<int8_t> seen;
    std::vector<int32_t> feature, bin;
    std::vector<uint32_t> counts;
    void reset(int32_t n_group, int32_t max_depth, int32_t nc) {
        per_tree = 2 << max_depth;
        n_classes = nc;
        seen.assign((size_t)n_group * per_tree, 0);
        feature.assign((size_t)n_group * per_tree, -1);
        bin.assign((size_t)n_group * per_tree, -1);
        counts.assign((size_t)n_group * per_tree * nc, 0u);
    }
    size_t at(int32_t g, int32_t id) const { return (size_t)g * per_tree + id; }
    void leaf(int32_t g, int32_t id, const uint32_t *c) {
        seen[at(g, id)] = 1;
        feature[at(g, id)] = bin[at(g, id)] = -1;
        std::copy(c, c + n_classes, counts.begin() + at(g, id) * n_classes);
    }
};

void sums(const uint32_t *c, int32_t nc, int64_t *n, int64_t *q) {
    *n = *q = 0;
    for (int32_t k = 0; k < nc; ++k) {
        *n += (int64_t)c[k];
        *q += (int64_t)c[k] * (int64_t)c[k];
    }
}

// the rule's feature subset of node `id` of tree `t`, ascending
void feature_subset(uint64_t seed, int32_t t, int32_t id, int32_t nf, int32_t m, int32_t *out) {
    if (m == nf) {
        for (int32_t f = 0; f < nf; ++f) out[f] = f;
        return;
    }
    std::pair<uint64_t, int32_t> key[CCDGPU_FOREST_MAX_FEATURES];
    const uint64_t node_key = ccd_train_fold(ccd_train_hash_a(seed, (uint64_t)t), (uint64_t)id);
    for (int32_t f = 0; f < nf; ++f) key[f] = {ccd_train_fold(node_key, (uint64_t)(1 + f)), f};
    std::partial_sort(key, key + m, key + nf);  // (pairs: equal keys go to the lower feature)
    for (int32_t j = 0; j < m; ++j) out[j] = key[j].second;
    std::sort(out, out + m);
}

}  // namespace

extern "C" {

int ccdgpu_forest_train(ccdgpu_ctx *c, const double *x, const int32_t *labels, int64_t n_rows, int32_t n_features,
                        int32_t n_classes, const double *edges, const int32_t *n_edges, const ccdgpu_train_params *p,
                        double *kernel_seconds) {
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    int rc = busy(c);
    if (rc) return rc;
    if ((rc = train_validate(x, labels, n_rows, n_features, n_classes, edges, n_edges, p))) return rc;
    const int32_t nf = n_features, nc = n_classes, m = train_features_per_node(nf, p);
    std::vector<int32_t> edge_off(nf + 1, 0);
    int32_t nb = 1;
    for (int32_t f = 0; f < nf; ++f) {
        edge_off[f + 1] = edge_off[f] + n_edges[f];
        nb = std::max(nb, n_edges[f] + 1);
    }
    const int64_t per_node = (int64_t)m * nb * nc;  // counters of one node
    const int64_t node_cap = p->max_depth == 0 ? 1 : std::min<int64_t>((int64_t)1 << (p->max_depth - 1), n_rows);
    int64_t group = TRAIN_GROUP_BYTES / (4 * n_rows + 4 * per_node * node_cap);
    if (const char *e = std::getenv("CCDGPU_TRAIN_GROUP_TREES")) group = std::atoll(e);
    group = std::max<int64_t>(1, std::min<int64_t>(group, std::min<int64_t>(p->n_trees, 65535)));

    HIPCHK(hipSetDevice(c->device));
    hipStream_t ax = c->aux;
    DevBuf<uint8_t> d_bins;
    DevBuf<double> d_x, d_edges;
    DevBuf<int32_t> d_labels, d_edge_off, d_n_edges, d_slot, d_tree_first, d_subset, d_split, d_child;
    DevBuf<uint32_t> d_hist, d_counts;
    Event ev[2];
    for (auto &e : ev) HIPCHK(e.create());
    const size_t nodes_cap = (size_t)(group * node_cap);
    if ((rc = d_bins.ensure((size_t)nf * (size_t)n_rows)) || (rc = d_x.ensure((size_t)(std::min(n_rows, TRAIN_SLAB_ROWS) * nf))) ||
        (rc = d_edges.ensure((size_t)edge_off[nf])) || (rc = d_labels.ensure((size_t)n_rows)) ||
        (rc = d_edge_off.ensure((size_t)nf + 1)) || (rc = d_n_edges.ensure((size_t)nf)) ||
        (rc = d_slot.ensure((size_t)group * (size_t)n_rows)) || (rc = d_tree_first.ensure((size_t)group + 1)) ||
        (rc = d_subset.ensure(nodes_cap * m)) || (rc = d_split.ensure(nodes_cap * 2)) || (rc = d_child.ensure(nodes_cap * 2)) ||
        (rc = d_hist.ensure(nodes_cap * (size_t)per_node)) || (rc = d_counts.ensure(nodes_cap * 2 * nc)))
        return rc;
    double secs = 0.0;
    auto elapsed = [&]() {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        secs += ms * 1e-3;
    };
    auto launch_failed = [&]() {
        (void)hipStreamSynchronize(ax);
        return fail(CCDGPU_EHIP, "training kernel launch failed");
    };

    // bins, once per call
    if (edge_off[nf] > 0)
        HIPCHK(hipMemcpyAsync(d_edges.p, edges, sizeof(double) * (size_t)edge_off[nf], hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(d_edge_off.p, edge_off.data(), sizeof(int32_t) * (size_t)(nf + 1), hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(d_n_edges.p, n_edges, sizeof(int32_t) * (size_t)nf, hipMemcpyHostToDevice, ax));
    HIPCHK(hipMemcpyAsync(d_labels.p, labels, sizeof(int32_t) * (size_t)n_rows, hipMemcpyHostToDevice, ax));
    for (int64_t r0 = 0; r0 < n_rows; r0 += TRAIN_SLAB_ROWS) {
        const int64_t n = std::min(TRAIN_SLAB_ROWS, n_rows - r0);
        HIPCHK(hipMemcpyAsync(d_x.p, x + r0 * nf, sizeof(double) * (size_t)(n * nf), hipMemcpyHostToDevice, ax));
        HIPCHK(hipEventRecord(ev[0], ax));
        if (ccdk_train_bin(d_x.p, r0, n, n_rows, nf, d_edges.p, d_edge_off.p, d_bins.p, ax)) return launch_failed();
        HIPCHK(hipEventRecord(ev[1], ax));
        HIPCHK(hipStreamSynchronize(ax));
        elapsed();
    }

    Trained out;
    out.n_features = nf;
    out.n_classes = nc;
    Grown grown;
    std::vector<Open> open, next;
    std::vector<int32_t> tree_first, subset, split, child;
    std::vector<uint32_t> counts;
    std::vector<std::pair<int32_t, int32_t>> stack;  // (node number, index of the parent in the output or -1)
    for (int32_t t0 = 0; t0 < p->n_trees; t0 += (int32_t)group) {
        const int32_t ng = (int32_t)std::min<int64_t>(group, p->n_trees - t0);
        grown.reset(ng, p->max_depth, nc);
        CcdTrainLevel lv{};
        lv.bins = d_bins.p;
        lv.labels = d_labels.p;
        lv.slot = d_slot.p;
        lv.tree_first = d_tree_first.p;
        lv.subset = d_subset.p;
        lv.hist = d_hist.p;
        lv.n_edges = d_n_edges.p;
        lv.n_rows = n_rows;
        lv.n_group_trees = ng;
        lv.m = m;
        lv.n_bins = nb;
        lv.n_classes = nc;
        lv.first_tree = t0;
        lv.bootstrap = p->bootstrap;
        lv.seed = p->seed;
        open.clear();
        for (int32_t g = 0; g < ng; ++g) open.push_back({g, 1});
        bool move_rows = false;  // the rows still stand at the previous level's nodes
        for (int32_t depth = 0; depth <= p->max_depth && !open.empty(); ++depth) {
            const int32_t nn = (int32_t)open.size();
            if ((size_t)nn > nodes_cap) return fail(CCDGPU_EHIP, "training: more open nodes than rows allow (internal)");
            // the level's node list (tree by tree) and the nodes' feature subsets
            tree_first.assign(ng + 1, 0);
            for (const Open &o : open) ++tree_first[o.g + 1];
            int32_t most = 0;
            for (int32_t g = 0; g < ng; ++g) {
                most = std::max(most, tree_first[g + 1]);
                tree_first[g + 1] += tree_first[g];
            }
            subset.resize((size_t)nn * m);
            for (int32_t i = 0; i < nn; ++i) feature_subset(p->seed, t0 + open[i].g, open[i].id, nf, m, &subset[(size_t)i * m]);
            const int64_t lds = (int64_t)most * per_node * 4;
            HIPCHK(hipEventRecord(ev[0], ax));
            if (move_rows) {  // (before the uploads below: it reads the previous level's lists)
                if (ccdk_train_assign(&lv, d_split.p, d_child.p, ax)) return launch_failed();
            } else if (ccdk_train_init(&lv, ax)) {
                return launch_failed();
            }
            lv.n_nodes = nn;
            HIPCHK(hipMemcpyAsync(d_tree_first.p, tree_first.data(), sizeof(int32_t) * (size_t)(ng + 1), hipMemcpyHostToDevice, ax));
            HIPCHK(hipMemcpyAsync(d_subset.p, subset.data(), sizeof(int32_t) * subset.size(), hipMemcpyHostToDevice, ax));
            if (ccdk_train_hist(&lv, lds <= CCD_TRAIN_LDS_BYTES ? (int32_t)lds : 0, ax) ||
                ccdk_train_split(&lv, p->min_instances_per_node, p->min_info_gain, d_split.p, d_counts.p, ax))
                return launch_failed();
            HIPCHK(hipEventRecord(ev[1], ax));
            split.resize((size_t)nn * 2);
            counts.resize((size_t)nn * 2 * nc);
            HIPCHK(hipMemcpyAsync(split.data(), d_split.p, sizeof(int32_t) * split.size(), hipMemcpyDeviceToHost, ax));
            HIPCHK(hipMemcpyAsync(counts.data(), d_counts.p, sizeof(uint32_t) * counts.size(), hipMemcpyDeviceToHost, ax));
            HIPCHK(hipStreamSynchronize(ax));
            elapsed();
            // leaves, splits and the next level's nodes
            next.clear();
            child.assign((size_t)nn * 2, -1);
            std::vector<uint32_t> side(nc);
            for (int32_t i = 0; i < nn; ++i) {
                const Open o = open[i];
                const uint32_t *cn = &counts[(size_t)i * 2 * nc], *cl = cn + nc;
                int64_t n, q;
                sums(cn, nc, &n, &q);
                if (depth == 0 && n == 0)
                    return fail(CCDGPU_EINVAL, "train: the bag of tree " + std::to_string(t0 + o.g) + " is empty");
                grown.leaf(o.g, o.id, cn);
                if (depth == p->max_depth || q == n * n || n < 2 * (int64_t)p->min_instances_per_node || split[2 * (size_t)i] < 0)
                    continue;
                grown.feature[grown.at(o.g, o.id)] = split[2 * (size_t)i];
                grown.bin[grown.at(o.g, o.id)] = split[2 * (size_t)i + 1];
                for (int32_t s = 0; s < 2; ++s) {
                    for (int32_t k = 0; k < nc; ++k) side[k] = s ? cn[k] - cl[k] : cl[k];
                    sums(side.data(), nc, &n, &q);
                    grown.leaf(o.g, 2 * o.id + s, side.data());
                    if (depth + 1 == p->max_depth || q == n * n || n < 2 * (int64_t)p->min_instances_per_node) continue;
                    child[2 * (size_t)i + s] = (int32_t)next.size();
                    next.push_back({o.g, 2 * o.id + s});
                }
            }
            if (next.empty()) break;
            // (the stream is idle: the copy lands before the next level's first launch reads it)
            HIPCHK(hipMemcpyAsync(d_child.p, child.data(), sizeof(int32_t) * child.size(), hipMemcpyHostToDevice, ax));
            HIPCHK(hipStreamSynchronize(ax));
            move_rows = true;
            open.swap(next);
        }
        // the group's trees in pre-order, left before right
        for (int32_t g = 0; g < ng; ++g) {
            out.root.push_back((int32_t)out.feature.size());
            stack.assign(1, {1, -1});
            while (!stack.empty()) {
                const int32_t id = stack.back().first, parent = stack.back().second;
                stack.pop_back();
                const size_t at = grown.at(g, id);
                if (!grown.seen[at]) return fail(CCDGPU_EHIP, "training: a tree lacks a node (internal)");
                const int32_t me = (int32_t)out.feature.size();
                if (parent >= 0) (id & 1 ? out.right : out.left)[parent] = me;
                const int32_t f = grown.feature[at];
                out.feature.push_back(f);
                out.threshold.push_back(f < 0 ? 0.0 : edges[edge_off[f] + grown.bin[at]]);
                out.left.push_back(-1);
                out.right.push_back(-1);
                const uint32_t *cn = &grown.counts[at * nc];
                int64_t n, q;
                sums(cn, nc, &n, &q);
                for (int32_t k = 0; k < nc; ++k) {
                    out.value.push_back((double)cn[k] / (double)n);
                    out.counts.push_back((int64_t)cn[k]);
                }
                if (f >= 0) {
                    stack.push_back({2 * id + 1, me});
                    stack.push_back({2 * id, me});  // popped first: the left subtree precedes the right
                }
            }
        }
    }
    out.has = true;
    c->trained = std::move(out);
    if (kernel_seconds) *kernel_seconds = secs;
    return 0;
}

int ccdgpu_trained_size(ccdgpu_ctx *c, int32_t *n_trees, int32_t *n_nodes) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (!n_trees || !n_nodes) return fail(CCDGPU_EINVAL, "NULL argument");
    if (!c->trained.has) return fail(CCDGPU_EINVAL, "no trained forest (ccdgpu_forest_train)");
    *n_trees = (int32_t)c->trained.root.size();
    *n_nodes = (int32_t)c->trained.feature.size();
    return 0;
}

int ccdgpu_trained_fetch(ccdgpu_ctx *c, ccdgpu_forest *into) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (!into) return fail(CCDGPU_EINVAL, "NULL argument");
    const Trained &t = c->trained;
    if (!t.has) return fail(CCDGPU_EINVAL, "no trained forest (ccdgpu_forest_train)");
    if (into->n_trees != (int32_t)t.root.size() || into->n_nodes != (int32_t)t.feature.size())
        return fail(CCDGPU_EINVAL, "trained_fetch: the arrays are for " + std::to_string(into->n_trees) + " trees and " +
                                       std::to_string(into->n_nodes) + " nodes, the trained forest has " +
                                       std::to_string(t.root.size()) + " and " + std::to_string(t.feature.size()));
    if (!into->root || !into->feature || !into->threshold || !into->left || !into->right || !into->value)
        return fail(CCDGPU_EINVAL, "trained_fetch: NULL array");
    std::copy(t.root.begin(), t.root.end(), const_cast<int32_t *>(into->root));
    std::copy(t.feature.begin(), t.feature.end(), const_cast<int32_t *>(into->feature));
    std::copy(t.threshold.begin(), t.threshold.end(), const_cast<double *>(into->threshold));
    std::copy(t.left.begin(), t.left.end(), const_cast<int32_t *>(into->left));
    std::copy(t.right.begin(), t.right.end(), const_cast<int32_t *>(into->right));
    std::copy(t.value.begin(), t.value.end(), const_cast<double *>(into->value));
    into->n_features = t.n_features;
    into->n_classes = t.n_classes;
    return 0;
}

int ccdgpu_trained_counts(ccdgpu_ctx *c, int64_t *counts, int64_t cap) {
    if (!c) return fail(CCDGPU_EINVAL, "NULL ctx");
    if (!counts) return fail(CCDGPU_EINVAL, "NULL argument");
    const Trained &t = c->trained;
    if (!t.has) return fail(CCDGPU_EINVAL, "no trained forest (ccdgpu_forest_train)");
    if (cap < (int64_t)t.counts.size())
        return fail(CCDGPU_EINVAL, "trained_counts: the array holds " + std::to_string(cap) + " counts, the trained forest has " +
                                       std::to_string(t.counts.size()));
    std::copy(t.counts.begin(), t.counts.end(), counts);
    return 0;
}

}  // extern "C"
