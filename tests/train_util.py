"""Reference for the random-forest training tests: the rule of include/ccdgpu.h in numpy (not part of
the product, which trains on the device only).  Integer counts, the rule's hash on uint64 arrays and
IEEE doubles, so the device's forest is compared with ``array_equal``."""
import numpy as np

import forest_util

U = np.uint64
GOLDEN = U(0x9E3779B97F4A7C15)
POISSON = np.array([1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777,
                    4294923276, 4294962463, 4294966817, 4294967252, 4294967292, 4294967295], dtype=np.uint64)


class EmptyBag(Exception):
    """The bag of tree ``args[0]`` is empty."""


def mix(z):
    z = np.asarray(z, dtype=U)
    with np.errstate(over='ignore'):
        z = z ^ (z >> U(30))
        z = z * U(0xBF58476D1CE4E5B9)
        z = z ^ (z >> U(27))
        z = z * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def fold(z, v):
    with np.errstate(over='ignore'):
        return mix(np.asarray(z, dtype=U) + GOLDEN + np.asarray(v, dtype=U))


def H(seed, a, b, c):
    with np.errstate(over='ignore'):
        return fold(fold(fold(mix(U(seed) + GOLDEN), a), b), c)


def weights(seed, t, n_rows, bootstrap):
    """w(t, r) for r = 0 .. n_rows-1, int64."""
    if not bootstrap:
        return np.ones(n_rows, dtype=np.int64)
    u = H(seed, t, np.arange(n_rows, dtype=U), 0) >> U(32)
    return (u[:, None] >= POISSON[None, :]).sum(axis=1).astype(np.int64)


def subset_size(n_features, m):
    """The m of the rule: 0 or 'sqrt' the smallest m with m * m >= n_features, 'all' every feature."""
    m = {'sqrt': 0, 'all': n_features}.get(m, m)
    if m == 0:
        while m * m < n_features:
            m += 1
    return min(m, n_features)


def subset(seed, t, node, n_features, m):
    """The m features of node ``node`` of tree ``t``, ascending: the smallest keys, ties to the lower f."""
    if m == n_features:
        return np.arange(n_features)
    keys = H(seed, t, node, 1 + np.arange(n_features, dtype=U))
    return np.sort(np.argsort(keys, kind='stable')[:m])


def bin_matrix(x, edges):
    """bin(r, f) = the number of e in edges[f] with e < x[r][f]."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([np.searchsorted(np.asarray(edges[f], dtype=np.float64), x[:, f], side='left')
                     for f in range(x.shape[1])], axis=1).astype(np.int64)


def _sums(c):
    c = [int(v) for v in c]
    return sum(c), sum(v * v for v in c)


def train(x, labels, edges, n_classes=None, n_trees=1, max_depth=5, features_per_node=0, min_instances_per_node=1,
          min_info_gain=0.0, bootstrap=1, seed=0):
    """The forest of the rule as forest_util.Arrays (trees in order, nodes in pre-order); EmptyBag(t)
    when tree t's bag is empty."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    n_rows, nf = x.shape
    C = int(y.max()) + 1 if n_classes is None else int(n_classes)
    edges = [np.asarray(e, dtype=np.float64) for e in edges]
    n_edges = np.array([e.shape[0] for e in edges])
    nb = int(n_edges.max()) + 1
    bins = bin_matrix(x, edges)
    m = subset_size(nf, features_per_node)
    root, feature, threshold, left, right, value = [], [], [], [], [], []

    def grow(t, w, node, depth, rows, c):
        me = len(feature)
        n, q = _sums(c)
        feature.append(-1)
        threshold.append(0.0)
        left.append(-1)
        right.append(-1)
        value.append(c.astype(np.float64) / np.float64(n))
        if depth == max_depth or q == n * n or n < 2 * min_instances_per_node:
            return me
        sub = subset(seed, t, node, nf, m)
        key = ((np.arange(m)[None, :] * nb + bins[rows][:, sub]) * C + y[rows][:, None]).reshape(-1)
        hist = np.bincount(key, weights=np.repeat(w[rows], m), minlength=m * nb * C).astype(np.int64).reshape(m, nb, C)
        cl = np.cumsum(hist, axis=1)   # [m][nb][C]: left counts of candidate (j, b)
        cr = c[None, None, :] - cl
        nl, nr = cl.sum(axis=2), cr.sum(axis=2)
        ql, qr = (cl * cl).sum(axis=2), (cr * cr).sum(axis=2)
        with np.errstate(divide='ignore', invalid='ignore'):
            score = ql.astype(np.float64) / nl.astype(np.float64) + qr.astype(np.float64) / nr.astype(np.float64)
            gain = (score - np.float64(q) / np.float64(n)) / np.float64(n)
        valid = ((np.arange(nb)[None, :] < n_edges[sub][:, None]) & (nl >= min_instances_per_node) &
                 (nr >= min_instances_per_node))
        valid &= np.where(valid, gain, -1.0) >= min_info_gain
        if not valid.any():
            return me
        flat = np.where(valid, score, -np.inf).reshape(-1)
        at = int(np.argmax(flat))  # the first of the largest: lowest f, then lowest b
        j, b = divmod(at, nb)
        f = int(sub[j])
        feature[me] = f
        threshold[me] = float(edges[f][b])
        go_left = bins[rows, f] <= b
        left[me] = grow(t, w, 2 * node, depth + 1, rows[go_left], cl[j, b])
        right[me] = grow(t, w, 2 * node + 1, depth + 1, rows[~go_left], cr[j, b])
        return me

    for t in range(n_trees):
        w = weights(seed, t, n_rows, bootstrap)
        rows = np.nonzero(w > 0)[0]
        if rows.size == 0:
            raise EmptyBag(t)
        c = np.bincount(y[rows], weights=w[rows], minlength=C).astype(np.int64)
        root.append(grow(t, w, 1, 0, rows, c))
    return forest_util.Arrays(root, feature, threshold, left, right, np.asarray(value), nf)


def equal(a, b):
    """The names of the ccdgpu_forest arrays in which forests ``a`` and ``b`` differ (shape, or any value)."""
    return [k for k in forest_util.ARRAYS
            if not np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k)))]


def first_trees(f, n):
    """The first ``n`` trees of forest ``f`` as forest_util.Arrays."""
    root = np.asarray(f.root)
    end = int(root[n]) if n < root.shape[0] else np.asarray(f.feature).shape[0]
    return forest_util.Arrays(root[:n], f.feature[:end], f.threshold[:end], f.left[:end], f.right[:end], f.value[:end],
                              f.n_features)


def perfect_case():
    """600 rows of 33 features drawn from 12 integer levels, label x[:, 7] // 3: (x, labels, edges)."""
    rng = np.random.default_rng(7)
    x = rng.integers(0, 12, size=(600, 33)).astype(np.float64)
    y = (x[:, 7] // 3).astype(np.int32)
    edges = [np.arange(11) + 0.5 for _ in range(33)]
    return x, y, edges
