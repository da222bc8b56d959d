"""ccdc.randomforest -- random-forest training and classification of segments: the ``rfrawp``
column (Spark-free mirror of reference ccdc/randomforest.py).

The reference trains a Spark ML RandomForestClassifier (500 trees, randomforest.py:25-39) on
``features.dataframe`` and keeps the model's ``rawPrediction`` per segment as ``rfrawp``
(array<float>; ``segment.join`` puts it on the segment rows).  Here ``train`` grows the forest on
the device over binned features, level by level, by the rule include/ccdgpu.h states
(ccd_train.hip through ``ccdgpu.Context.train_forest``; ``find_splits`` chooses the bins, on the
host or, given a context, on the device: ccd_splits.hip), and a forest -- trained or imported, plain
arrays either way -- is evaluated on the device
(ccd_forest.hip through ``ccdgpu.Context.classify`` / ``classify_rows``); there is no CPU path.
A trained forest is judged by ``oob`` -- every row scored on the device only by the trees whose bag
it was not in (``Context.forest_oob``), summed up by ``evaluation`` -- by ``feature_importances``, and by
``permutation_importances``: the out-of-bag votes a shuffled feature loses (``Context.forest_permutation``).

rawPrediction of a row is the sum over the trees, in tree order, of the reached leaf's normalised
class distribution, indexed by label.  A Spark ``RandomForestClassificationModel`` maps to the
arrays tree by tree (``model.trees``): an InternalNode gives ``feature = split.featureIndex``,
``threshold = split.threshold`` (ContinuousSplit: ``x <= threshold`` goes left) and its two
children; a LeafNode gives ``feature = -1`` and ``value = impurityStats.stats / sum(stats)``;
numbering each tree's nodes in pre-order satisfies the child > parent rule of the check.
"""
import collections
import ctypes
import math

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from ccdc import features

KEYS = ['cx', 'cy', 'px', 'py', 'sday', 'eday']
_ARRAYS = ('root', 'feature', 'threshold', 'left', 'right', 'value')


class Forest(object):
    """A forest as the arrays of ccdgpu_forest: root [n_trees], feature / threshold / left /
    right [n_nodes] (feature < 0 marks a leaf), value [n_nodes][n_classes] (leaves' normalised
    class distributions).  A forest trained here (``ccdgpu.Context.train_forest``) also carries
    ``counts`` int64 [n_nodes][n_classes] (the weighted class counts ``value`` is made of), ``seed`` and
    ``bootstrap``: what ``oob``, ``permutation_importances`` and ``feature_importances`` need.  They are
    None on any other forest; ``save`` keeps those a forest has."""

    counts = seed = bootstrap = None

    def __init__(self, root, feature, threshold, left, right, value, n_features):
        from ccdgpu import abi
        self._struct, arrays = abi.forest_struct(root, feature, threshold, left, right, value, n_features)
        self.root, self.feature, self.threshold, self.left, self.right, self.value = arrays
        self.n_features = int(n_features)

    n_trees = property(lambda self: int(self.root.shape[0]))
    n_nodes = property(lambda self: int(self.feature.shape[0]))
    n_classes = property(lambda self: int(self.value.shape[1]))

    def struct(self):
        """The abi.Forest over this forest's arrays (valid while the forest is alive)."""
        return self._struct

    def check(self):
        """ccdgpu_forest_check (no device needed): ValueError with the library's message."""
        import ccdgpu
        if ccdgpu.lib().ccdgpu_forest_check(ctypes.byref(self._struct)) != 0:
            raise ValueError(ccdgpu.last_error())
        return self

    @property
    def max_depth(self):
        """Branches from a root to the deepest leaf (ccdgpu_forest_depth)."""
        import ccdgpu
        d = ctypes.c_int32(0)
        if ccdgpu.lib().ccdgpu_forest_depth(ctypes.byref(self._struct), ctypes.byref(d)) != 0:
            raise ValueError(ccdgpu.last_error())
        return d.value

    @classmethod
    def from_arrays(cls, root, feature, threshold, left, right, value, n_features):
        """Forest from array-likes, validated by the library's check."""
        return cls(root, feature, threshold, left, right, value, n_features).check()

    @classmethod
    def from_sklearn(cls, rf):
        """Forest of a fitted sklearn RandomForestClassifier (or any ensemble of single-output
        DecisionTreeClassifiers in ``estimators_``).  The class vector is Spark's, indexed by
        label: ``classes_`` must be non-negative integers, n_classes = max(label) + 1, labels the
        training set lacks are zero columns."""
        classes = np.asarray(rf.classes_)
        if classes.ndim != 1 or getattr(rf, 'n_outputs_', 1) != 1:
            raise ValueError('from_sklearn needs a single-output classifier')
        if classes.dtype.kind == 'b' or not (classes.dtype.kind in 'iu' or
                                             (classes.dtype.kind == 'f' and np.all(classes == np.floor(classes)))):
            raise ValueError('class labels must be non-negative integers, got %r' % (classes.tolist(),))
        labels = classes.astype(np.int64)
        if labels.size == 0 or labels.min() < 0:
            raise ValueError('class labels must be non-negative integers, got %r' % (classes.tolist(),))
        n_classes = int(labels.max()) + 1
        root, feature, threshold, left, right, value = [], [], [], [], [], []
        base = 0
        for est in rf.estimators_:
            t = est.tree_
            n = int(t.node_count)
            leaf = t.children_left[:n] < 0
            v = np.asarray(t.value[:n, 0, :], dtype=np.float64)
            if v.shape[1] != labels.size:
                raise ValueError('a tree has %d classes, the ensemble %d' % (v.shape[1], labels.size))
            v = v / v.sum(axis=1, keepdims=True)
            full = np.zeros((n, n_classes), dtype=np.float64)
            full[:, labels] = v
            root.append(base)
            feature.append(np.where(leaf, -1, t.feature[:n]).astype(np.int32))
            threshold.append(np.where(leaf, 0.0, t.threshold[:n]))
            left.append(np.where(leaf, -1, t.children_left[:n] + base).astype(np.int32))
            right.append(np.where(leaf, -1, t.children_right[:n] + base).astype(np.int32))
            value.append(full)
            base += n
        return cls.from_arrays(np.asarray(root, np.int32), np.concatenate(feature), np.concatenate(threshold),
                               np.concatenate(left), np.concatenate(right), np.concatenate(value),
                               int(rf.n_features_in_))

    def save(self, path):
        """Write the arrays as .npz (``path`` as given to numpy.savez: a name gets '.npz'), with ``seed``,
        ``bootstrap`` and ``counts`` where the forest has them, so that a trained forest can be judged later."""
        extra = {}
        if self.seed is not None:
            extra['seed'] = np.uint64(self.seed)
        if self.bootstrap is not None:
            extra['bootstrap'] = np.bool_(self.bootstrap)
        if self.counts is not None:
            extra['counts'] = np.asarray(self.counts, dtype=np.int64)
        np.savez(path, n_features=np.int32(self.n_features), **extra, **{k: getattr(self, k) for k in _ARRAYS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            f = cls.from_arrays(*[z[k] for k in _ARRAYS], n_features=int(z['n_features']))
            if 'seed' in z.files:
                f.seed = int(z['seed'])
            if 'bootstrap' in z.files:
                f.bootstrap = bool(z['bootstrap'])
            if 'counts' in z.files:
                f.counts = z['counts'].astype(np.int64)
            return f


def find_splits(matrix, max_bins=32, context=None):
    """Bin edges of the columns of ``matrix`` [n_rows][n_features] (finite values): a list of
    increasing float64 arrays, one per feature -- Spark ML's rule for continuous features
    (RandomForest.findSplitsForContinuousFeature, with every row a sample).

    Per column, d_0 < d_1 < .. are its distinct values and n_i their counts.  With at most
    ``max_bins`` distinct values the edges are the midpoints (d_i + d_{i+1}) / 2 of consecutive
    distinct values (none for a constant column).  Otherwise there are at most ``max_bins - 1``
    count-quantile cut points: with stride = n_rows / max_bins, target = stride and c the running
    count n_0 + .. + n_{i-1}, for i = 1, 2, .. in order: if |c - target| < |c + n_i - target| the
    midpoint (d_{i-1} + d_i) / 2 is an edge and target grows by stride; then c grows by n_i.  A
    midpoint equal to the edge before it (neighbouring doubles) is dropped, so the edges strictly
    increase.  2 <= max_bins <= 64 (the device's bin matrix is uint8 with at most 63 edges).

    Without a ``context`` the edges are computed here on the host (a sort per column).  With a
    ``ccdgpu.Context`` they are found on the device (``Context.find_splits``: ccd_splits.hip, the same
    rule over positions of the sorted columns) and are equal to the host's array by array."""
    if context is not None:
        if np.ndim(matrix) != 2:
            raise ValueError('matrix must be [n_rows][n_features], got %r' % (np.shape(matrix),))
        return context.find_splits(matrix, max_bins)
    x = np.asarray(matrix, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError('matrix must be [n_rows][n_features], got %r' % (x.shape,))
    if not 2 <= int(max_bins) <= 64:
        raise ValueError('max_bins must be in 2 .. 64, got %r' % (max_bins,))
    if not np.all(np.isfinite(x)):
        raise ValueError('matrix holds non-finite values')
    n_splits = int(max_bins) - 1
    out = []
    for f in range(x.shape[1]):
        d, n = np.unique(x[:, f], return_counts=True)
        mid = (d[:-1] + d[1:]) / 2.0
        if d.shape[0] - 1 > n_splits:
            stride = x.shape[0] / float(n_splits + 1)
            before = np.cumsum(n)[:-1].tolist()  # the count below d_i, i = 1 ..
            count = n[1:].tolist()
            take, target = [], stride
            for i, (c, k) in enumerate(zip(before, count)):
                if abs(c - target) < abs(c + k - target):
                    take.append(i)
                    target += stride
            mid = mid[take]
        if mid.shape[0] > 1:
            mid = mid[np.concatenate(([True], mid[1:] > mid[:-1]))]
        out.append(np.ascontiguousarray(mid))
    return out


def train(dataframe, n_trees=500, max_depth=5, max_bins=32, features_per_node='auto', min_instances_per_node=1,
          min_info_gain=0.0, bootstrap=True, seed=0, context=None, oob=False, permutation=False, perm_seed=0,
          splits='host'):
    """Train the forest of the reference's ``train`` (randomforest.py:25-39: 500 trees over
    ``features.dataframe``) on the device and return it as a ``Forest``.  ``dataframe`` is the table of
    ``features.dataframe``: its ``label`` column (trends[0]) the classes, n_classes = max(label) + 1, its
    ``features`` column the 33 features.  Rows with a null label or a non-finite feature are dropped;
    the forest's ``rows_dropped`` / ``rows_trained`` say how many went and stayed.  features_per_node
    'auto' is every feature for one tree and 'sqrt' otherwise, as Spark's ``featureSubsetStrategy``;
    'sqrt', 'all' or a count choose directly.  The bins are ``find_splits(matrix, max_bins)``, computed on
    the host with ``splits`` 'host' and on the context the forest is trained on with 'device' (the same
    edges either way); the other
    parameters are those of ccdgpu_train_params (include/ccdgpu.h states the rule).  With ``oob`` the
    forest also gets ``forest.oob``: the out-of-bag ``Evaluation`` over the kept rows, in their order
    (``oob`` below; it needs ``bootstrap`` and leaves the trained forest set as the context's).  With
    ``permutation`` it gets ``forest.permutation``: the ``PermutationImportances`` over the kept rows
    under ``perm_seed`` (``permutation_importances`` below; the same conditions)."""
    if splits not in ('host', 'device'):
        raise ValueError("splits must be 'host' or 'device', got %r" % (splits,))
    if oob and not bootstrap:
        raise ValueError('oob needs bootstrap: without it every bag is every row and no tree is out of bag')
    if permutation and not bootstrap:
        raise ValueError('permutation needs bootstrap: without it every bag is every row and no tree is out of bag')
    x = features.matrix(dataframe)
    label = pc.cast(dataframe['label'], pa.float64()).to_numpy(zero_copy_only=False)
    keep = np.isfinite(label) & np.all(np.isfinite(x), axis=1)
    x, y = np.ascontiguousarray(x[keep]), label[keep]
    if x.shape[0] == 0:
        raise ValueError('no row with a label and finite features to train on (%d rows dropped)' % keep.shape[0])
    if np.any(y < 0) or np.any(y != np.floor(y)):
        raise ValueError('labels must be non-negative integers')
    if features_per_node == 'auto':
        features_per_node = 'all' if int(n_trees) == 1 else 'sqrt'
    ctx = _context(context)
    edges = find_splits(x, max_bins, context=ctx if splits == 'device' else None)
    forest = ctx.train_forest(
        x, y.astype(np.int32), edges, n_trees=n_trees, max_depth=max_depth,
        features_per_node=features_per_node, min_instances_per_node=min_instances_per_node, min_info_gain=min_info_gain,
        bootstrap=bool(bootstrap), seed=seed)
    forest.rows_trained, forest.rows_dropped = int(x.shape[0]), int(keep.shape[0] - x.shape[0])
    if oob:
        forest.oob = _oob(forest, x, y.astype(np.int32), context=ctx)
    if permutation:
        forest.permutation = permutation_importances(forest, x, y.astype(np.int32), perm_seed=perm_seed, context=ctx)
    return forest


def _context(context):
    import ccdgpu
    return context or ccdgpu.default_context()


Evaluation = collections.namedtuple('Evaluation', ['raw', 'n_oob', 'predicted', 'confusion', 'rows_scored', 'accuracy',
                                                   'producers', 'users'])
Evaluation.__doc__ = """What ``evaluation`` returns: ``raw`` float32 [n][n_classes] and ``n_oob`` int32 [n] as given (the
trees that scored each row), ``predicted`` int64 [n] (-1: not scored), ``confusion`` int64
[label][predicted] over the scored rows, ``rows_scored``, ``accuracy``, and per class ``producers``
(recall: of the rows with that label, the share predicted so) and ``users`` (precision: of the rows
predicted so, the share with that label); a ratio with a zero denominator is NaN."""


def evaluation(raw, n_scored, labels, n_classes):
    """The ``Evaluation`` of raw predictions ``raw`` [n][n_classes] against ``labels`` [n] in 0 ..
    n_classes-1, over the rows with ``n_scored`` > 0 (pure numpy).  The predicted class of a scored row
    is the argmax of its float32 values, a tie going to the lower class; a row no tree scored is
    predicted -1 and counts nowhere."""
    raw = np.asarray(raw, dtype=np.float32)
    n_oob = np.asarray(n_scored, dtype=np.int32).reshape(-1)
    y = np.asarray(labels).reshape(-1)
    nc = int(n_classes)
    if raw.ndim != 2 or raw.shape[1] != nc or not raw.shape[0] == n_oob.shape[0] == y.shape[0]:
        raise ValueError('raw must be [n][%d] with n_scored [n] and labels [n], got %r, %r and %r'
                         % (nc, raw.shape, n_oob.shape, y.shape))
    if y.size and (np.any(y != np.floor(y)) or y.min() < 0 or y.max() >= nc):
        raise ValueError('labels must be integers in 0 .. %d' % (nc - 1))
    y = y.astype(np.int64)
    scored = n_oob > 0
    predicted = np.where(scored, np.argmax(raw, axis=1), -1).astype(np.int64)  # argmax: the first of the largest
    confusion = np.bincount(y[scored] * nc + predicted[scored], minlength=nc * nc).astype(np.int64).reshape(nc, nc)
    hit = np.diagonal(confusion).astype(np.float64)
    rows_scored = int(scored.sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        accuracy = float(np.float64(hit.sum()) / np.float64(rows_scored))
        producers = hit / confusion.sum(axis=1).astype(np.float64)
        users = hit / confusion.sum(axis=0).astype(np.float64)
    return Evaluation(raw, n_oob, predicted, confusion, rows_scored, accuracy, producers, users)


def oob(forest, x, labels, seed=None, first_row=0, context=None):
    """The out-of-bag ``Evaluation`` of ``forest`` over x [n_rows][n_features] and ``labels`` [n_rows]:
    every row is scored on the device only by the trees whose bag it was not in (include/ccdgpu.h states
    the rule; ccd_forest.hip through ``ccdgpu.Context.forest_oob``), so the accuracy is an estimate for
    rows the forest has not seen, which the accuracy on the training rows is not.  x and labels are the
    training matrix and its labels in the training order -- or rows [first_row, first_row + n_rows) of
    them: the bag of a row is a function of (seed, tree, row index) and nothing is stored for it.
    ``seed`` None takes the forest's own (a forest trained here has one).  Sets ``forest`` as the
    context's forest.  ValueError for a forest trained without bootstrap (every bag is every row, so no
    tree is out of bag), or without a seed when none is given."""
    if forest.bootstrap is not None and not forest.bootstrap:
        raise ValueError('the forest was trained without bootstrap: every bag is every row and no tree is out of bag')
    if seed is None:
        seed = forest.seed
    if seed is None:
        raise ValueError('the forest has no seed (it was not trained here): give the seed its bags were drawn with')
    ctx = _context(context)
    ctx.set_forest(forest)
    raw, n_oob = ctx.forest_oob(x, seed, first_row)
    return evaluation(raw, n_oob, labels, forest.n_classes)


_oob = oob  # (``train`` has a flag of this name)


PermutationImportances = collections.namedtuple(
    'PermutationImportances', ['importances', 'importances_std', 'class_importances', 'trees_used', 'oob_rows', 'correct',
                               'lost', 'gained'])
PermutationImportances.__doc__ = """What ``permutation_importances`` returns: ``importances`` float64 [n_features] (the mean
over the trees of the share of a tree's out-of-bag rows whose right vote a shuffled column loses, less the
share it gains: R randomForest's MeanDecreaseAccuracy, unscaled), ``importances_std`` (its sample standard
deviation over the trees), ``class_importances`` float64 [n_classes][n_features] (the same over the rows
of one label), ``trees_used`` (the trees with an out-of-bag row), and the integer counts ``oob_rows``,
``correct`` [n_trees][n_classes], ``lost``, ``gained`` [n_trees][n_features][n_classes] as given."""


def permutation_summary(oob_rows, correct, lost, gained):
    """The ``PermutationImportances`` of the counts of ``Context.forest_permutation`` (host, Python floats
    over integer sums).  With N_t = sum_k oob_rows[t][k], the trees with N_t == 0 are left out and
    ``trees_used`` counts the rest; d[t][f] = float(sum_k lost[t][f][k] - sum_k gained[t][f][k]) /
    float(N_t); importances[f] is the d[t][f] added in tree order, divided by trees_used;
    importances_std[f] the square root of the sum in tree order of (d[t][f] - importances[f])^2 over
    trees_used - 1, NaN below two trees.  class_importances[k][f] is the same mean, over the trees with
    oob_rows[t][k] > 0, of float(lost[t][f][k] - gained[t][f][k]) / float(oob_rows[t][k]); a class no
    tree saw gets NaN, and without a tree every figure is NaN."""
    oob_rows, correct = np.asarray(oob_rows, dtype=np.int64), np.asarray(correct, dtype=np.int64)
    lost, gained = np.asarray(lost, dtype=np.int64), np.asarray(gained, dtype=np.int64)
    if oob_rows.ndim != 2 or correct.shape != oob_rows.shape or lost.ndim != 3 or gained.shape != lost.shape or \
            (lost.shape[0], lost.shape[2]) != oob_rows.shape:
        raise ValueError('oob_rows and correct must be [n_trees][n_classes], lost and gained [n_trees][n_features][n_classes], '
                         'got %r, %r, %r and %r' % (oob_rows.shape, correct.shape, lost.shape, gained.shape))
    nt, nf, nc = lost.shape
    rows, net = oob_rows.tolist(), (lost - gained).tolist()
    nan = float('nan')
    used = [t for t in range(nt) if sum(rows[t]) > 0]
    imp, std = np.full(nf, nan), np.full(nf, nan)
    per_class = np.full((nc, nf), nan)
    for f in range(nf):
        d = [float(sum(net[t][f])) / float(sum(rows[t])) for t in used]
        if d:
            total = 0.0
            for v in d:
                total += v
            imp[f] = total / len(d)
        if len(d) > 1:
            ss = 0.0
            for v in d:
                ss += (v - imp[f]) * (v - imp[f])
            std[f] = math.sqrt(ss / (len(d) - 1))
        for k in range(nc):
            saw = [t for t in used if rows[t][k] > 0]
            if saw:
                total = 0.0
                for t in saw:
                    total += float(net[t][f][k]) / float(rows[t][k])
                per_class[k][f] = total / len(saw)
    return PermutationImportances(imp, std, per_class, len(used), oob_rows, correct, lost, gained)


def permutation_importances(forest, x, labels, seed=None, perm_seed=0, context=None):
    """The out-of-bag permutation importances of ``forest`` over x [n_rows][n_features] and ``labels``
    [n_rows], the whole training matrix and its labels in training order: for every tree, the rows out
    of its bag are voted on as they are and with each feature's column shuffled in turn, on the device
    (include/ccdgpu.h states the rule; ccd_forest.hip through ``ccdgpu.Context.forest_permutation``), and
    ``permutation_summary`` turns the counts into ``PermutationImportances``.  Unlike
    ``feature_importances`` this is judged on rows a tree has not seen, and it does not favour the
    features that offer many split points.  ``seed`` None takes the forest's own; ``perm_seed`` chooses
    the shuffles.  Sets ``forest`` as the context's forest.  ValueError for a forest trained without
    bootstrap, or without a seed when none is given."""
    if forest.bootstrap is not None and not forest.bootstrap:
        raise ValueError('the forest was trained without bootstrap: every bag is every row and no tree is out of bag')
    if seed is None:
        seed = forest.seed
    if seed is None:
        raise ValueError('the forest has no seed (it was not trained here): give the seed its bags were drawn with')
    ctx = _context(context)
    ctx.set_forest(forest)
    return permutation_summary(*ctx.forest_permutation(x, labels, seed, perm_seed))


def feature_importances(forest):
    """Spark ML's ``featureImportances`` of a forest trained here, float64 [n_features], on the host from
    ``forest.counts`` (ValueError without them).  With c_k a node's counts, n = sum c_k and q = sum c_k^2
    (integers), the training rule's numerator ``score - q/n`` is gain * n, Spark's term of a split.  Per
    tree, over its internal nodes in pre-order, imp[feature] +=
    ((double)qL/(double)nL + (double)qR/(double)nR) - (double)q/(double)n with L and R the node's
    children; s = the sum of imp in feature order, added one by one; if s > 0, imp /= s.  The trees'
    vectors are added in tree order and the total is normalised the same way."""
    if forest.counts is None:
        raise ValueError('the forest has no counts (it was not trained here): feature_importances needs forest.counts')
    counts = np.asarray(forest.counts, dtype=np.int64)
    if counts.shape != (forest.n_nodes, forest.n_classes):
        raise ValueError('counts must be [%d][%d], got %r' % (forest.n_nodes, forest.n_classes, counts.shape))
    n = [int(v) for v in counts.sum(axis=1)]
    q = [int(v) for v in (counts * counts).sum(axis=1)]
    feature, left, right = forest.feature.tolist(), forest.left.tolist(), forest.right.tolist()
    if 0 in n:
        raise ValueError('node %d has no counts' % n.index(0))

    def normalised(imp):
        s = 0.0
        for v in imp.tolist():
            s += v
        return imp / s if s > 0 else imp

    total = np.zeros(forest.n_features, dtype=np.float64)
    for r in forest.root.tolist():
        imp = np.zeros(forest.n_features, dtype=np.float64)
        stack = [r]
        while stack:
            i = stack.pop()
            if feature[i] < 0:
                continue
            a, b = left[i], right[i]
            imp[feature[i]] += (float(q[a]) / float(n[a]) + float(q[b]) / float(n[b])) - float(q[i]) / float(n[i])
            stack.append(b)
            stack.append(a)  # popped first: the left subtree precedes the right
        total += normalised(imp)
    return normalised(total)


def predictions(aux, segments, forest, context=None):
    """Raw predictions of the segments that have a model: an Arrow table cx, cy, px, py, sday,
    eday, rfrawp (the reference's predictions dataframe, joined to the segments by ``join``).
    The features are ``features.join`` / ``independent`` / ``matrix`` of the aux and segment
    tables; the forest runs on the device (``Context.classify``)."""
    t = features.join({'aux': aux, 'ccd': segments})
    t = t.filter(pc.is_valid(t['chprob']))  # pyccd.default's rows have no model to classify
    ctx = _context(context)
    ctx.set_forest(forest)
    raw = ctx.classify(features.matrix(features.independent(t)))
    from ccdc import sink
    return t.select(KEYS).append_column('rfrawp', sink._list_col(raw, np.ones(raw.shape[0], dtype=bool)))


def join(segments, predictions):
    """Arrow counterpart of segment.join (segment.py:103-116): inner join on cx, cy, px, py,
    sday, eday; the segments' rfrawp column replaced by the predictions'.  Rows keep the
    segments' order."""
    s = segments.select(KEYS).append_column('_s', pa.array(np.arange(segments.num_rows, dtype=np.int64)))
    p = predictions.select(KEYS).cast(segments.select(KEYS).schema)  # (a table built elsewhere: the segments' key types)
    p = p.append_column('_p', pa.array(np.arange(predictions.num_rows, dtype=np.int64)))
    j = s.join(p, keys=KEYS, join_type='inner').sort_by([('_s', 'ascending')])
    out = segments.take(j['_s'])
    raw = predictions['rfrawp'].take(j['_p'])
    i = out.schema.get_field_index('rfrawp')
    return out.set_column(i, out.schema.field(i), pc.cast(raw, out.schema.field(i).type))


def classify_chips_tables(chips, aux_of, forest, params=None, context=None, width=100):
    """``pyccd.detect_chips_tables`` with the segment tables' rfrawp filled: each batch's rows are
    gathered into feature vectors and classified on the device right behind its detection
    (``Context.classify_rows``), rows without a model staying null.  aux_of(cx, cy) gives the
    chip's [n_pix][5] aux values (dem, aspect, slope, mpw, posidex), pixels in row-major order."""
    import ccdgpu
    from ccdc import pyccd, sink
    ctx = _context(context)
    ctx.set_forest(forest)
    state = {}

    def on_batch(ctx, keys, n_pix):
        aux = np.concatenate([np.asarray(aux_of(cx, cy), dtype=np.float64).reshape(n_pix, 5) for cx, cy in keys])
        state['raw'], state['at'] = ctx.classify_rows(aux), 0

    out = []
    for ctx, c, (cx, cy), dates, n_pix in pyccd._run_chips(chips, params, ctx, on_batch=on_batch):
        u = ctx.fetch(c)  # procedure / QA error check
        if u.error_pixel >= 0:
            raise ccdgpu.QAValueError('unsupported QA value at pixel %d of chip (%d, %d)' % (u.error_pixel, cx, cy))
        off, rows, mask = ctx.fetch_rows(c, cx, cy, width)
        a = state['at']
        state['at'] = a + rows.shape[0]  # the batch's rows are chip-major
        out.append(((cx, cy), sink.tables(cx, cy, dates, off, rows, mask, rfrawp=state['raw'][a:a + rows.shape[0]])))
    return out
