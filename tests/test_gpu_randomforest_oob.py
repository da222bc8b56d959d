"""The out-of-bag walk on the device (ccd_forest_oob in ccd_forest.hip through Context.forest_oob) and
the trained forest's counts against the numpy restatement of the rule (tests/oob_util.py): every
comparison is array_equal on both outputs.  The kernel cases use generated forests at the smallest
shapes at which each path runs: both launch shapes around their block sizes, every class-count
template width and its boundary, several LDS chunks, a tree walked from global memory, a second slab."""
import ctypes

import numpy as np
import pytest

import ccdgpu
import forest_util
import oob_util
import train_util as tu
from ccdc import randomforest
from ccdc.randomforest import Forest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = ccdgpu.Context(0)
    yield c
    c.close()


def _rows(seed, n, nf):
    return np.random.default_rng(seed).normal(size=(n, nf))


def _same(ctx, f, x, seed, first_row=0):
    ctx.set_forest(Forest.from_arrays(*f.args()))
    raw, n = ctx.forest_oob(x, seed, first_row)
    ref_raw, ref_n = oob_util.oob(f, x, seed, first_row)
    assert raw.dtype == np.float32 and raw.shape == ref_raw.shape and n.dtype == np.int32 and n.shape == ref_n.shape
    assert np.array_equal(n, ref_n)
    assert np.array_equal(raw, ref_raw)
    return raw, n


@pytest.mark.parametrize('n_rows,nf', [(1, 5), (63, 5), (64, 5), (65, 5), (511, 5), (512, 5), (513, 5), (1000, 5),
                                       (255, 64), (256, 64), (257, 64)])
def test_row_counts(ctx, n_rows, nf):
    assert ccdgpu.lib().ccdk_forest_threads(nf) == (512 if nf == 5 else 256)
    x = _rows(n_rows, n_rows, nf)
    _same(ctx, forest_util.random_forest(3, 7, 4, nf, 3, rows=x), x, seed=n_rows)


@pytest.mark.parametrize('n_classes', [1, 2, 3, 4, 5, 9, 10, 16, 17, 32])
def test_class_counts(ctx, n_classes):
    x = _rows(n_classes, 130, 6)
    _same(ctx, forest_util.random_forest(n_classes, 9, 4, 6, n_classes), x, seed=4)


def test_several_chunks(ctx):
    f = forest_util.random_forest(11, 70, 5, 33, 9, p_leaf=0.0)
    cap = ccdgpu.lib().ccdk_forest_chunk_cap(33)
    assert 70 * (63 * 16 + 32 * 9 * 8) > 2 * cap  # the forest's blobs need more than two chunks
    _same(ctx, f, _rows(12, 700, 33), seed=6)


def test_a_tree_walked_from_global_memory(ctx):
    small = forest_util.random_forest(13, 1, 3, 33, 9)
    big = forest_util.random_forest(14, 1, 11, 33, 9, p_leaf=0.0)
    last = forest_util.random_forest(15, 1, 3, 33, 9)
    assert big.feature.shape[0] == 4095 and 4095 * 16 + 2048 * 9 * 8 > ccdgpu.lib().ccdk_forest_chunk_cap(33)
    root, parts = [], []
    for f in (small, big, last):
        base = sum(p.feature.shape[0] for p in parts)
        root.append(base)
        parts.append(f)
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])
    shift = lambda k: np.concatenate([np.where(getattr(p, k) >= 0, getattr(p, k) + b, -1) for p, b in zip(parts, root)])
    f = forest_util.Arrays(root, cat('feature'), cat('threshold'), shift('left'), shift('right'), cat('value'), 33)
    raw, n = _same(ctx, f, _rows(16, 700, 33), seed=8)
    assert set(n.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize('seed', [0, 1, 2 ** 63 + 5, 2 ** 64 - 1])
def test_seeds(ctx, seed):
    x = _rows(21, 300, 5)
    _same(ctx, forest_util.random_forest(22, 12, 4, 5, 4), x, seed=seed)


def test_the_largest_hash_index(ctx):
    x = _rows(23, 200, 5)
    f = forest_util.random_forest(24, 8, 4, 5, 3)
    top = ccdgpu.abi.TRAIN_MAX_ROWS
    _same(ctx, f, x, seed=9, first_row=top - 200)
    with pytest.raises(ccdgpu.CcdGpuError, match='first_row') as err:
        ctx.forest_oob(x, 9, top - 199)
    assert err.value.code == ccdgpu.abi.E_INVAL


def test_chunked_calls_are_slices_of_the_whole(ctx):
    x = _rows(25, 1000, 5)
    f = forest_util.random_forest(26, 10, 4, 5, 3)
    raw, n = _same(ctx, f, x, seed=10)
    for a, b in ((0, 300), (1, 513), (511, 1000), (700, 701)):
        part_raw, part_n = ctx.forest_oob(x[a:b], 10, first_row=a)
        assert np.array_equal(part_raw, raw[a:b]) and np.array_equal(part_n, n[a:b])


def test_rows_beyond_one_slab(ctx):
    """2^20 + 3 rows: the second slab is three rows long and is launched with its own first_row."""
    n = (1 << 20) + 3
    x = _rows(27, n, 1)
    f = forest_util.random_forest(28, 3, 1, 1, 2, p_leaf=0.0)
    raw, count = _same(ctx, f, x, seed=11)
    assert count[-3:].tolist() == oob_util.oob(f, x[-3:], 11, first_row=1 << 20)[1].tolist()
    assert ctx.oob_seconds > 0.0


def test_nan_goes_right(ctx):
    x = _rows(29, 100, 4)
    x[::3, 1] = np.nan
    x[5] = np.nan
    f = forest_util.random_forest(30, 6, 3, 4, 3, p_leaf=0.0)
    raw, n = _same(ctx, f, x, seed=12)
    one = forest_util.Arrays([0], [1, -1, -1], [0.0, 0.0, 0.0], [1, -1, -1], [2, -1, -1], [[0, 0], [1, 0], [0, 1]], 4)
    raw, n = _same(ctx, one, x, seed=12)
    scored = n > 0
    assert scored[::3].any() and np.all(raw[::3][scored[::3]] == [0.0, 1.0])


def test_no_rows_and_a_wrong_feature_count(ctx):
    ctx.set_forest(Forest.from_arrays(*forest_util.random_forest(31, 2, 2, 4, 3).args()))
    raw, n = ctx.forest_oob(np.zeros((0, 4)), 1)
    assert raw.shape == (0, 3) and n.shape == (0,)
    with pytest.raises(ValueError):
        ctx.forest_oob(np.zeros((3, 5)), 1)
    with pytest.raises(ccdgpu.CcdGpuError, match='first_row'):
        ctx.forest_oob(np.zeros((3, 4)), 1, first_row=-1)


@pytest.fixture(scope='module')
def perfect():
    return tu.perfect_case()


@pytest.mark.parametrize('n_trees,unscored', [(1, 382), (2, 255), (3, 173), (20, 0)])
def test_rows_without_an_out_of_bag_tree(ctx, perfect, n_trees, unscored):
    x, y, edges = perfect
    forest = ctx.train_forest(x, y, edges, n_trees=n_trees, max_depth=5, features_per_node='all', seed=3)
    ref_raw, ref_n = oob_util.oob(forest, x, 3)
    assert int((ref_n == 0).sum()) == unscored
    e = randomforest.oob(forest, x, y, context=ctx)
    assert np.array_equal(e.n_oob, ref_n) and np.array_equal(e.raw, ref_raw)
    none = e.n_oob == 0
    assert np.all(e.raw[none] == 0.0) and np.all(e.predicted[none] == -1) and np.all(e.predicted[~none] >= 0)
    assert e.rows_scored == 600 - unscored == e.confusion.sum()
    if n_trees == 20:
        assert e.accuracy == 1.0 and np.array_equal(e.predicted, y)
    ctx.clear_forest()


@pytest.mark.parametrize('bootstrap', [0, 1])
def test_counts(ctx, monkeypatch, bootstrap):
    rng = np.random.default_rng(33)
    x = rng.normal(size=(500, 12))
    y = np.clip(np.floor((x[:, 0] + 0.7 * x[:, 6] + 0.3 * rng.normal(size=500) + 2.0) / 4.0 * 9), 0, 8).astype(np.int32)
    edges = randomforest.find_splits(x, 16)
    par = dict(n_classes=9, n_trees=6, max_depth=5, seed=5, bootstrap=bootstrap)
    forest = ctx.train_forest(x, y, edges, **par)
    assert forest.counts.dtype == np.int64 and forest.counts.shape == (forest.n_nodes, 9)
    assert (forest.seed, forest.bootstrap) == (5, bool(bootstrap))
    assert np.array_equal(forest.counts, oob_util.node_counts(forest, x, y, 5, bootstrap, 9))
    n = forest.counts.sum(axis=1, keepdims=True)
    assert np.array_equal(forest.value, forest.counts.astype(np.float64) / n.astype(np.float64))
    monkeypatch.setenv('CCDGPU_TRAIN_GROUP_TREES', '1')
    one = ctx.train_forest(x, y, edges, **par)
    assert tu.equal(one, forest) == [] and np.array_equal(one.counts, forest.counts)
    # the library's own refusals
    L = ccdgpu.lib()
    short = np.zeros(forest.counts.size - 1, dtype=np.int64)
    assert L.ccdgpu_trained_counts(ctx._ctx, short.ctypes.data, short.size) == ccdgpu.abi.E_INVAL
    assert 'trained_counts' in ccdgpu.last_error()
    fresh = ccdgpu.Context(0)
    try:
        assert L.ccdgpu_trained_counts(fresh._ctx, short.ctypes.data, short.size) == ccdgpu.abi.E_INVAL
        assert 'no trained forest' in ccdgpu.last_error()
    finally:
        fresh.close()


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_importances(ctx, perfect):
    x, y, edges = perfect
    forest = ctx.train_forest(x, y, edges, n_trees=5, max_depth=5, features_per_node='all', seed=3)
    imp = randomforest.feature_importances(forest)
    assert imp.dtype == np.float64 and imp.shape == (33,)
    assert imp[7] == 1.0 and np.all(np.delete(imp, 7) == 0.0)
    assert _ulps(imp, oob_util.importances(forest, forest.counts)).max() <= 4
    forest = ctx.train_forest(x, y, edges, n_trees=20, max_depth=5, features_per_node='sqrt', seed=3)
    imp = randomforest.feature_importances(forest)
    ref = oob_util.importances(forest, oob_util.node_counts(forest, x, y, 3, 1, forest.n_classes))
    assert _ulps(imp, ref).max() <= 4
    assert int(np.argmax(imp)) == 7  # (the restatement: 0.553 there, 0.030 for the runner-up)
    assert abs(imp.sum() - 1.0) < 33 * 2.0 ** -52  # 33 correctly rounded quotients of one sum


def test_state_is_left_alone(ctx):
    x = _rows(35, 300, 33)
    y = (np.arange(300) % 4).astype(np.int32)
    ctx.train_forest(x, y, randomforest.find_splits(x, 8), n_classes=4, n_trees=3, max_depth=3, seed=1)
    L = ccdgpu.lib()
    size = lambda: tuple(v.value for v in _size(L, ctx))
    before = size()
    f = forest_util.random_forest(36, 6, 4, 33, 9)
    _same(ctx, f, x, seed=13)
    assert np.array_equal(ctx.classify(x), forest_util.walk(f, x))
    assert size() == before
    ctx.clear_forest()
    with pytest.raises(ccdgpu.CcdGpuError, match='no forest set') as err:
        ctx.forest_oob(x, 13)
    assert err.value.code == ccdgpu.abi.E_INVAL
    ctx._forest_shape = (33, 9)  # past the binding's own refusal: the library's
    try:
        with pytest.raises(ccdgpu.CcdGpuError, match='no forest set') as err:
            ctx.forest_oob(x, 13)
        assert err.value.code == ccdgpu.abi.E_INVAL
    finally:
        ctx._forest_shape = None


def _size(L, ctx):
    nt, nn = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.ccdgpu_trained_size(ctx._ctx, ctypes.byref(nt), ctypes.byref(nn)) == 0
    return nt, nn


def test_train_with_oob_over_the_features_dataframe(ctx):
    """ccdc.randomforest.train(dataframe, oob=True) over features.dataframe of a chip the device detected:
    forest.oob is the out-of-bag evaluation over the kept rows, in their order."""
    from ccdc import chipmunk, features, pyccd
    from ccdgpu import synth
    from test_gpu_features import CX, CY, _aux
    n_pix = 100
    d, s, q = synth.chip(synth.config(5), 4, 0, n_pix)
    order = np.argsort(d)[::-1]
    d, s, q = d[order], s[:, :, order], q[:, order]
    (key, t), = pyccd.detect_chips_tables(chipmunk.chip_response(CX, CY, d, s, q))
    table = features.dataframe(_aux(n_pix), t['segment'])
    m = features.matrix(table)
    label = np.asarray(table['label'].to_pylist(), dtype=np.float64)
    keep = np.all(np.isfinite(m), axis=1) & np.isfinite(label)
    x, y = m[keep], label[keep].astype(np.int32)
    plain = randomforest.train(table, n_trees=6, max_depth=4, max_bins=16, seed=3, context=ctx)
    assert not hasattr(plain, 'oob')
    forest = randomforest.train(table, n_trees=6, max_depth=4, max_bins=16, seed=3, context=ctx, oob=True)
    assert tu.equal(forest, plain) == []
    e = forest.oob
    assert e.confusion.sum() == e.rows_scored <= forest.rows_trained == x.shape[0]
    ref_raw, ref_n = oob_util.oob(forest, x, 3)
    assert np.array_equal(e.raw, ref_raw) and np.array_equal(e.n_oob, ref_n)
    assert e.rows_scored == int((ref_n > 0).sum()) > 0
    assert e.confusion.shape == (forest.n_classes, forest.n_classes)
    ctx.clear_forest()
