"""Reference for the permutation-importance tests: the rule of include/ccdgpu.h in numpy, done the plain
way (not part of the product, whose walk runs on the device only) -- for every tree and every feature
the column is substituted and all the tree's out-of-bag rows are walked again, whether or not their
paths test the feature -- and the importances as a plain loop."""
import math

import numpy as np

import oob_util
import train_util as tu

U = np.uint64
HASH_C = 1 << 32


def pair(perm_seed, t, f, n):
    """(a, b) of the permutation of column f for tree t over n rows."""
    k = int(tu.H(perm_seed, t, f, HASH_C))
    a = (k & 0xffffffff) % n
    while math.gcd(a, n) != 1:
        a = (a + 1) % n
    return a, (k >> 32) % n


def donors(perm_seed, t, f, n):
    """uint64 [n]: donor(t, f, r) = (a*r + b) mod n for r = 0 .. n-1."""
    a, b = pair(perm_seed, t, f, n)
    return (U(a) * np.arange(n, dtype=U) + U(b)) % U(n)


def votes(f, root, x):
    """int64 [n]: per row of x, the lowest class with the largest value at the leaf it reaches from ``root``."""
    feature, threshold = np.asarray(f.feature), np.asarray(f.threshold)
    left, right, value = np.asarray(f.left), np.asarray(f.right), np.asarray(f.value, dtype=np.float64)
    node = np.full(x.shape[0], root, dtype=np.int64)
    while True:
        idx = np.nonzero(feature[node] >= 0)[0]
        if idx.size == 0:
            break
        at = node[idx]
        with np.errstate(invalid='ignore'):
            go_left = x[idx, feature[at]] <= threshold[at]  # NaN compares false: right
        node[idx] = np.where(go_left, left[at], right[at])
    return np.argmax(value[node], axis=1)  # the first of the largest


def tested(f, root):
    """The set of features tree ``root`` tests."""
    feature, left, right = np.asarray(f.feature), np.asarray(f.left), np.asarray(f.right)
    seen, stack = set(), [int(root)]
    while stack:
        i = stack.pop()
        if feature[i] >= 0:
            seen.add(int(feature[i]))
            stack += [int(left[i]), int(right[i])]
    return seen


def counts(f, x, y, seed, perm_seed=0):
    """(oob_rows, correct [n_trees][n_classes], lost, gained [n_trees][n_features][n_classes]), int64."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    n, nf = x.shape
    roots = np.asarray(f.root).tolist()
    nt, nc = len(roots), np.asarray(f.value).shape[1]
    oob_rows, correct = np.zeros((nt, nc), np.int64), np.zeros((nt, nc), np.int64)
    lost, gained = np.zeros((nt, nf, nc), np.int64), np.zeros((nt, nf, nc), np.int64)
    for t, root in enumerate(roots):
        rows = np.nonzero(oob_util.out_of_bag(seed, t, 0, n))[0] if n else np.zeros(0, np.int64)
        yo = y[rows]
        base = votes(f, root, x[rows]) == yo
        oob_rows[t] = np.bincount(yo, minlength=nc)
        correct[t] = np.bincount(yo[base], minlength=nc)
        for c in range(nf):
            xp = x[rows].copy()
            xp[:, c] = x[donors(perm_seed, t, c, n)[rows].astype(np.int64), c]
            perm = votes(f, root, xp) == yo
            lost[t, c] = np.bincount(yo[base & ~perm], minlength=nc)
            gained[t, c] = np.bincount(yo[~base & perm], minlength=nc)
    return oob_rows, correct, lost, gained


def importances(oob_rows, lost, gained):
    """(importances, importances_std [n_features], class_importances [n_classes][n_features], trees_used) by
    the arithmetic ccdc.randomforest.permutation_summary states, one tree and one term at a time."""
    nt, nf, nc = lost.shape
    nan = np.float64('nan')
    imp, std, per_class = [nan] * nf, [nan] * nf, [[nan] * nf for _ in range(nc)]
    used = [t for t in range(nt) if int(oob_rows[t].sum()) > 0]
    for f in range(nf):
        d = []
        for t in used:
            net = sum(int(lost[t, f, k]) for k in range(nc)) - sum(int(gained[t, f, k]) for k in range(nc))
            d.append(np.float64(net) / np.float64(int(oob_rows[t].sum())))
        if d:
            s = np.float64(0.0)
            for v in d:
                s = s + v
            imp[f] = s / np.float64(len(d))
        if len(d) > 1:
            s = np.float64(0.0)
            for v in d:
                s = s + (v - imp[f]) * (v - imp[f])
            std[f] = np.sqrt(s / np.float64(len(d) - 1))
        for k in range(nc):
            s, m = np.float64(0.0), 0
            for t in used:
                if oob_rows[t, k] > 0:
                    s = s + np.float64(int(lost[t, f, k]) - int(gained[t, f, k])) / np.float64(int(oob_rows[t, k]))
                    m += 1
            if m:
                per_class[k][f] = s / np.float64(m)
    return np.array(imp), np.array(std), np.array(per_class).reshape(nc, nf), len(used)
