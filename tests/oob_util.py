"""Reference for the out-of-bag tests: the rule of include/ccdgpu.h in numpy (not part of the product,
whose walk runs on the device only) -- the out-of-bag raw prediction, the nodes' weighted class counts
derived by routing the rows (not from the trainer's histograms), and the importances as a plain loop."""
import numpy as np

import forest_util
import train_util as tu

U = np.uint64
CUT = tu.POISSON[0]


def out_of_bag(seed, t, first_row, n_rows):
    """bool [n_rows]: u = H(seed, t, r, 0) >> 32 is below P[0] for r = first_row + i."""
    r = np.arange(first_row, first_row + n_rows, dtype=U)
    return (tu.H(seed, t, r, 0) >> U(32)) < CUT


def oob(f, x, seed, first_row=0):
    """(oob_raw float32 [n][n_classes], n_oob int32 [n]) of rows x through forest ``f``: per tree, in
    order, the rows out of its bag get the reached leaf's class vector added in double."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    raw = np.zeros((n, np.asarray(f.value).shape[1]), dtype=np.float64)
    count = np.zeros(n, dtype=np.int32)
    for t in range(np.asarray(f.root).shape[0]):
        out = np.nonzero(out_of_bag(seed, t, first_row, n))[0]
        one = forest_util.Arrays(np.asarray(f.root)[t:t + 1], f.feature, f.threshold, f.left, f.right, f.value, f.n_features)
        raw[out] += forest_util.walk_raw(one, x[out])  # (one tree: 0.0 + its leaf's vector, exact)
        count[out] += 1
    return raw.astype(np.float32), count


def node_counts(f, x, y, seed, bootstrap, n_classes):
    """int64 [n_nodes][n_classes]: every row in tree t's bag goes down the tree by its thresholds and adds
    its weight w(t, r), under its label, at every node it passes."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    feature, threshold = np.asarray(f.feature), np.asarray(f.threshold)
    left, right = np.asarray(f.left), np.asarray(f.right)
    counts = np.zeros((feature.shape[0], n_classes), dtype=np.int64)
    for t, root in enumerate(np.asarray(f.root).tolist()):
        w = tu.weights(seed, t, x.shape[0], bootstrap)
        rows = np.nonzero(w > 0)[0]
        node = np.full(rows.shape[0], root, dtype=np.int64)
        while rows.size:
            np.add.at(counts, (node, y[rows]), w[rows])
            go = feature[node] >= 0
            rows, node = rows[go], node[go]
            node = np.where(x[rows, feature[node]] <= threshold[node], left[node], right[node])
    return counts


def importances(f, counts):
    """The rule of ccdc.randomforest.feature_importances, node by node."""
    counts = np.asarray(counts)
    nf = f.n_features
    feature, left, right = np.asarray(f.feature), np.asarray(f.left), np.asarray(f.right)

    def nq(i):
        c = [int(v) for v in counts[i]]
        return np.float64(sum(c)), np.float64(sum(v * v for v in c))

    def visit(i, imp):  # pre-order
        if feature[i] < 0:
            return
        (n, q), (nl, ql), (nr, qr) = nq(i), nq(left[i]), nq(right[i])
        imp[feature[i]] = imp[feature[i]] + ((ql / nl + qr / nr) - q / n)
        visit(left[i], imp)
        visit(right[i], imp)

    def normalise(imp):
        s = np.float64(0.0)
        for k in range(nf):
            s = s + imp[k]
        if s > 0:
            for k in range(nf):
                imp[k] = imp[k] / s

    total = [np.float64(0.0)] * nf
    for root in np.asarray(f.root).tolist():
        imp = [np.float64(0.0)] * nf
        visit(root, imp)
        normalise(imp)
        for k in range(nf):
            total[k] = total[k] + imp[k]
    normalise(total)
    return np.array(total, dtype=np.float64)
