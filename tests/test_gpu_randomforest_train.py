"""Random-forest training on the device (ccd_train.hip through Context.train_forest) against the
numpy restatement of the rule (tests/train_util.py): every comparison is array_equal on all six
forest arrays.  Shapes are the smallest at which each path runs: one and several histogram blocks,
levels whose counters fit LDS and levels that take the global path, one and several tree groups."""
import numpy as np
import pytest

import ccdgpu
import forest_util
import train_util as tu
from ccdc import randomforest
from ccdc.randomforest import Forest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = ccdgpu.Context(0)
    yield c
    c.close()


def _data(seed, n_rows, nf, nc, constant=()):
    """Continuous features; the label follows the first features, with noise, over nc classes."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n_rows, nf))
    for f in constant:
        x[:, f] = 1.25
    s = x[:, 0] + (0.7 * x[:, nf // 2] if nf > 1 else 0.0) + 0.3 * rng.normal(size=n_rows)
    y = np.clip(np.floor((s + 2.0) / 4.0 * nc), 0, nc - 1).astype(np.int32)
    return x, y


def _same(ctx, x, y, edges, n_classes=None, **par):
    got = ctx.train_forest(x, y, edges, n_classes=n_classes, **par)
    ref = tu.train(x, y, edges, n_classes=n_classes, **par)
    assert got.n_trees == ref.root.shape[0] and got.n_nodes == ref.feature.shape[0]
    assert tu.equal(got, ref) == []
    return got, ref


@pytest.mark.parametrize('n_rows', [1, 63, 64, 65, 257, 1000])
def test_row_counts(ctx, n_rows):
    x, y = _data(n_rows, n_rows, 5, 3)
    _same(ctx, x, y, randomforest.find_splits(x, 16), n_classes=3, n_trees=3, max_depth=4, bootstrap=0, seed=n_rows)


@pytest.mark.parametrize('n_classes', [1, 2, 9, 32])
def test_class_counts(ctx, n_classes):
    x, y = _data(n_classes, 400, 6, n_classes)
    got, _ = _same(ctx, x, y, randomforest.find_splits(x, 16), n_classes=n_classes, n_trees=4, max_depth=4, seed=2)
    if n_classes == 1:  # every tree a single leaf
        assert got.feature.tolist() == [-1] * 4 and got.value.tolist() == [[1.0]] * 4


@pytest.mark.parametrize('nf', [1, 33, 64])
def test_feature_counts_with_a_constant_column(ctx, nf):
    x, y = _data(nf, 300, nf, 4, constant=(nf - 1,))
    edges = randomforest.find_splits(x, 8)
    assert len(edges[nf - 1]) == 0
    got, _ = _same(ctx, x, y, edges, n_classes=4, n_trees=3, max_depth=4, features_per_node='all' if nf == 33 else 0, seed=5)
    assert nf - 1 not in got.feature.tolist()


@pytest.mark.parametrize('max_bins', [2, 32, 64])
def test_edges_per_feature(ctx, max_bins):
    x, y = _data(max_bins, 500, 4, 3)
    edges = randomforest.find_splits(x, max_bins)
    assert [len(e) for e in edges] == [max_bins - 1] * 4  # 1, 31 and 63 edges
    _same(ctx, x, y, edges, n_classes=3, n_trees=3, max_depth=5, features_per_node='all', seed=1)


@pytest.mark.parametrize('max_depth', [0, 1, 5, 10])
def test_depths(ctx, max_depth):
    """Depth 10 over 1000 rows of continuous features: its deeper levels hold more nodes per tree than
    the LDS counters take (48 KiB: 25 nodes of 3 features x 32 bins x 5 classes), so they run the
    global path."""
    x, y = _data(40 + max_depth, 1000, 8, 5)
    got, ref = _same(ctx, x, y, randomforest.find_splits(x, 32), n_classes=5, n_trees=2, max_depth=max_depth, seed=7)
    assert got.max_depth <= max_depth
    if max_depth == 10:
        assert _widest_level(ref) * 3 * 32 * 5 * 4 > 49152


def _widest_level(f):
    """The most internal nodes any tree of forest ``f`` has at one depth."""
    widest = 0
    for r in f.root.tolist():
        level = [r]
        while level:
            level = [n for n in level if f.feature[n] >= 0]
            widest = max(widest, len(level))
            level = [c for n in level for c in (int(f.left[n]), int(f.right[n]))]
    return widest


@pytest.mark.parametrize('n_trees', [1, 7, 20])
def test_tree_counts(ctx, n_trees):
    x, y = _data(3, 257, 10, 4)
    _same(ctx, x, y, randomforest.find_splits(x, 16), n_classes=4, n_trees=n_trees, max_depth=4, seed=11)


@pytest.mark.parametrize('par', [dict(bootstrap=0), dict(bootstrap=1), dict(features_per_node='all'),
                                 dict(features_per_node='sqrt'), dict(features_per_node=3, bootstrap=0),
                                 dict(min_instances_per_node=5), dict(min_info_gain=0.01),
                                 dict(min_instances_per_node=5, min_info_gain=0.01, bootstrap=0, features_per_node='all')],
                         ids=lambda p: '-'.join('%s=%s' % kv for kv in p.items()))
def test_parameter_variants(ctx, par):
    x, y = _data(8, 600, 12, 4)
    _same(ctx, x, y, randomforest.find_splits(x, 16), n_classes=4, n_trees=5, max_depth=6, seed=13, **par)


def test_identical_columns_go_to_the_lower_index(ctx):
    x, y = _data(21, 400, 4, 3)
    x[:, 2] = x[:, 0]
    edges = randomforest.find_splits(x, 16)
    got, _ = _same(ctx, x, y, edges, n_classes=3, n_trees=4, max_depth=5, features_per_node=4, seed=3)
    assert 0 in got.feature.tolist() and 2 not in got.feature.tolist()


def test_symmetric_bins_go_to_the_lower_bin(ctx):
    """Three values with classes 0, 1, 0 and equal counts at the ends: the cuts below and above the
    middle value score the same; the lower one is chosen."""
    x = np.repeat([0.0, 1.0, 2.0], [50, 30, 50]).reshape(-1, 1)
    y = np.repeat([0, 1, 0], [50, 30, 50]).astype(np.int32)
    got, ref = _same(ctx, x, y, [[0.5, 1.5]], n_classes=2, n_trees=1, max_depth=1, bootstrap=0)
    assert got.feature.tolist() == [0, -1, -1] and got.threshold[0] == 0.5


@pytest.mark.parametrize('classes', [1, 2])
def test_contention_on_one_counter(ctx, classes):
    """1000 rows in one bin: of one class (every add of a tree lands on one counter; the root is pure),
    and of two (no candidate has a right side: a leaf by the candidates' rule)."""
    x = np.full((1000, 1), 3.0)
    y = (np.arange(1000) % classes).astype(np.int32)
    got, _ = _same(ctx, x, y, [[5.0]], n_classes=2, n_trees=3, max_depth=3, seed=4)
    assert got.feature.tolist() == [-1] * 3


def test_counters_are_wider_than_16_bits(ctx):
    x = np.concatenate([np.zeros(66500), np.ones(3500)]).reshape(-1, 1)
    y = (np.arange(70000) % 100 == 0).astype(np.int32)
    y[66500:] = 1
    assert int(((x[:, 0] < 0.5) & (y == 0)).sum()) > 65535
    got, _ = _same(ctx, x, y, [[0.5]], n_classes=2, n_trees=1, max_depth=1, bootstrap=0)
    assert got.feature.tolist() == [0, -1, -1]
    _same(ctx, x, y, [[0.5]], n_classes=2, n_trees=2, max_depth=1, bootstrap=1, seed=6)


def test_rows_beyond_one_binning_slab(ctx):
    """2^20 + 5 rows: the rows go up and are binned in two slabs, the second one five rows long; every
    count of the two-level tree holds those rows (the last five are the only ones of class 2)."""
    n = (1 << 20) + 5
    x = np.random.default_rng(31).normal(size=(n, 2))
    y = (x[:, 1] > 0.3).astype(np.int32)
    x[-5:, 0], x[-5:, 1], y[-5:] = 9.0, 1.0, 2
    got, _ = _same(ctx, x, y, [[-0.5, 8.0], [0.3]], n_classes=3, n_trees=1, max_depth=2, bootstrap=0, features_per_node='all')
    assert got.value[:, 2].max() == 1.0  # a leaf of exactly those five rows


def test_first_trees_do_not_depend_on_the_tree_count_or_the_grouping(ctx, monkeypatch):
    x, y = _data(3, 257, 10, 4)
    edges = randomforest.find_splits(x, 16)
    par = dict(n_classes=4, max_depth=5, seed=11)
    twenty = ctx.train_forest(x, y, edges, n_trees=20, **par)
    seven = ctx.train_forest(x, y, edges, n_trees=7, **par)
    assert tu.equal(tu.first_trees(twenty, 7), seven) == []
    monkeypatch.setenv('CCDGPU_TRAIN_GROUP_TREES', '3')  # groups of 3, 3, .., 2 trees
    assert tu.equal(ctx.train_forest(x, y, edges, n_trees=20, **par), twenty) == []
    monkeypatch.setenv('CCDGPU_TRAIN_GROUP_TREES', '1')
    assert tu.equal(ctx.train_forest(x, y, edges, n_trees=7, **par), seven) == []


def test_an_empty_bag_is_refused_by_tree(ctx):
    x, y = np.array([[1.0, 2.0]]), np.array([1], dtype=np.int32)
    # a seed whose first empty bag of this one row is not the first tree's
    seed, t = next((s, t) for s in range(64) for t in [int(np.argmin([tu.weights(s, k, 1, 1)[0] > 0 for k in range(32)]))]
                   if t >= 2)
    with pytest.raises(tu.EmptyBag) as ref:
        tu.train(x, y, [[0.0], []], n_classes=2, n_trees=t + 1, seed=seed)
    assert ref.value.args[0] == t
    with pytest.raises(ccdgpu.CcdGpuError, match=r'bag of tree %d is empty' % t) as err:
        ctx.train_forest(x, y, [[0.0], []], n_classes=2, n_trees=t + 1, seed=seed)
    assert err.value.code == ccdgpu.abi.E_INVAL
    _same(ctx, x, y, [[0.0], []], n_classes=2, n_trees=t, seed=seed)  # the trees before it are single leaves
    with pytest.raises(ccdgpu.CcdGpuError, match=r'labels\[0\]'):
        ctx.train_forest(x, y, [[0.0], []], n_classes=1)


def test_train_then_classify(ctx):
    """Training does not touch the context's forest; the trained forest passes the check, and set as
    the context's forest classifies its training rows as the walk of the same arrays does."""
    x, y = _data(17, 500, 33, 9)
    before = forest_util.random_forest(5, 6, 4, 33, 9)
    ctx.set_forest(Forest.from_arrays(*before.args()))
    raw_before = ctx.classify(x)
    forest = ctx.train_forest(x, y, randomforest.find_splits(x, 32), n_classes=9, n_trees=10, max_depth=5, seed=2)
    assert np.array_equal(ctx.classify(x), raw_before)
    assert np.array_equal(raw_before, forest_util.walk(before, x))
    forest.check()
    ctx.set_forest(forest)
    raw = ctx.classify(x)
    assert np.array_equal(raw, forest_util.walk(forest, x))
    assert (np.argmax(raw, axis=1) == y).mean() > 0.5  # (9 classes: chance is far below)
    ctx.clear_forest()


def test_perfect_tree_on_the_device(ctx):
    x, y, edges = tu.perfect_case()
    got, _ = _same(ctx, x, y, edges, n_trees=1, max_depth=3, features_per_node=33, bootstrap=0)
    assert got.n_nodes == 7 and sorted(got.feature.tolist()) == [-1, -1, -1, -1, 7, 7, 7]
    assert np.array_equal(np.argmax(forest_util.walk_raw(got, x), axis=1), y)


def test_train_over_the_features_dataframe(ctx):
    """ccdc.randomforest.train over features.dataframe of a chip the device detected: rows without a
    model (null features) are dropped and counted, the forest equals the restatement over the kept
    rows, and ``predictions`` with it closes the loop."""
    from ccdc import chipmunk, features, pyccd
    from ccdgpu import synth
    from test_gpu_features import CX, CY, _aux
    n_pix = 100
    d, s, q = synth.chip(synth.config(5), 4, 0, n_pix)
    order = np.argsort(d)[::-1]
    d, s, q = d[order], s[:, :, order], q[:, order]
    (key, t), = pyccd.detect_chips_tables(chipmunk.chip_response(CX, CY, d, s, q))
    aux = _aux(n_pix)
    table = features.dataframe(aux, t['segment'])
    m = features.matrix(table)
    label = np.asarray(table['label'].to_pylist(), dtype=np.float64)
    keep = np.all(np.isfinite(m), axis=1) & np.isfinite(label)
    assert keep.sum() > n_pix // 2
    forest = randomforest.train(table, n_trees=6, max_depth=4, max_bins=16, seed=3, context=ctx)
    assert (forest.rows_trained, forest.rows_dropped) == (int(keep.sum()), int((~keep).sum()))
    x, y = m[keep], label[keep].astype(np.int32)
    ref = tu.train(x, y, randomforest.find_splits(x, 16), n_trees=6, max_depth=4, seed=3)
    assert tu.equal(forest, ref) == [] and forest.n_classes == int(y.max()) + 1 and forest.n_features == 33
    one = randomforest.train(table, n_trees=1, max_depth=3, max_bins=16, seed=3, context=ctx)  # 'auto': all features
    assert tu.equal(one, tu.train(x, y, randomforest.find_splits(x, 16), n_trees=1, max_depth=3, features_per_node=33, seed=3)) == []
    pred = randomforest.predictions(aux, t['segment'], forest, context=ctx)
    assert 0 < pred.num_rows <= table.num_rows
    raw = np.asarray(pred['rfrawp'].to_pylist(), dtype=np.float32)
    assert raw.shape[1] == forest.n_classes and np.allclose(raw.sum(axis=1), 6.0, atol=1e-4)
    ctx.clear_forest()
