"""Reference for the random-forest tests: the walk of include/ccdgpu.h in numpy (not part of the
product, which has no CPU path) and seeded forests as plain arrays."""
import numpy as np

ARRAYS = ('root', 'feature', 'threshold', 'left', 'right', 'value')


def walk_raw(f, x):
    """The double sums [n_rows][n_classes] of rows x [n_rows][n_features] through forest ``f``
    (anything with the ccdgpu_forest arrays as attributes): per row, trees in order, the reached
    leaf's class vector added in double.  x <= threshold goes left; NaN compares false and goes
    right."""
    x = np.asarray(x, dtype=np.float64)
    feature, threshold = np.asarray(f.feature), np.asarray(f.threshold)
    left, right, value = np.asarray(f.left), np.asarray(f.right), np.asarray(f.value, dtype=np.float64)
    n = x.shape[0]
    raw = np.zeros((n, value.shape[1]), dtype=np.float64)
    for r in np.asarray(f.root):
        node = np.full(n, r, dtype=np.int64)
        while True:
            idx = np.nonzero(feature[node] >= 0)[0]
            if idx.size == 0:
                break
            at = node[idx]
            with np.errstate(invalid='ignore'):
                go_left = x[idx, feature[at]] <= threshold[at]
            node[idx] = np.where(go_left, left[at], right[at])
        raw += value[node]
    return raw


def walk(f, x):
    """rfrawp: walk_raw rounded to float32 (round to nearest)."""
    return walk_raw(f, x).astype(np.float32)


class Arrays(object):
    """The ccdgpu_forest arrays of a generated forest."""

    def __init__(self, root, feature, threshold, left, right, value, n_features):
        self.root = np.asarray(root, dtype=np.int32)
        self.feature = np.asarray(feature, dtype=np.int32)
        self.threshold = np.asarray(threshold, dtype=np.float64)
        self.left = np.asarray(left, dtype=np.int32)
        self.right = np.asarray(right, dtype=np.int32)
        self.value = np.asarray(value, dtype=np.float64)
        self.n_features = int(n_features)

    def args(self):
        return [getattr(self, k) for k in ARRAYS] + [self.n_features]


def concatenated(parts):
    """The forests ``parts`` (same features and classes) as one: their trees in order, child indices shifted."""
    base = np.cumsum([0] + [p.feature.shape[0] for p in parts[:-1]])
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])
    shift = lambda k: np.concatenate([np.where(getattr(p, k) >= 0, getattr(p, k) + b, -1) for p, b in zip(parts, base)])
    root = np.concatenate([p.root + b for p, b in zip(parts, base)])
    return Arrays(root, cat('feature'), cat('threshold'), shift('left'), shift('right'), cat('value'), parts[0].n_features)


def random_forest(seed, n_trees, max_depth, n_features, n_classes, p_leaf=0.15, rows=None):
    """Seeded forest, nodes in pre-order (child > parent).  A node above max_depth becomes a leaf
    with probability p_leaf (p_leaf=0: complete trees; max_depth=0: single-leaf trees).  Leaf
    values are random normalised class distributions; thresholds are standard normal, or -- with
    rows [n][n_features] -- the tested feature's value in a random row, so that rows meet
    thresholds they equal exactly."""
    rng = np.random.default_rng(seed)
    root, feature, threshold, left, right = [], [], [], [], []
    for _ in range(n_trees):
        root.append(len(feature))
        stack = [(-1, 0, 0)]  # (parent, side, depth)
        while stack:
            parent, side, depth = stack.pop()
            n = len(feature)
            if parent >= 0:
                (right if side else left)[parent] = n
            if depth >= max_depth or rng.random() < p_leaf:
                feature.append(-1)
                threshold.append(0.0)
            else:
                f = int(rng.integers(n_features))
                feature.append(f)
                threshold.append(float(rows[rng.integers(rows.shape[0]), f]) if rows is not None else float(rng.normal()))
                stack.append((n, 1, depth + 1))
                stack.append((n, 0, depth + 1))  # popped first: the left subtree precedes the right
            left.append(-1)
            right.append(-1)
    v = rng.random((len(feature), n_classes)) + 1e-3
    v /= v.sum(axis=1, keepdims=True)
    return Arrays(root, feature, threshold, left, right, v, n_features)
