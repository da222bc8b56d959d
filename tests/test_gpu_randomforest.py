"""Random-forest inference on the HIP path (ccd_forest.hip through ccdgpu.Context.classify /
classify_rows) against the numpy walk of tests/forest_util.py.  The walk fixes the order of every
addition, so the comparisons are exact (array_equal on the float32 output) except against
sklearn's predict_proba, whose own summation order is not fixed."""
import ctypes

import numpy as np
import pyarrow.compute as pc
import pytest

import ccdgpu
import forest_util
import golden_util
import parity_util
from ccdgpu import abi
from ccdc import features, randomforest
from ccdc.randomforest import Forest

pytestmark = pytest.mark.gpu

N_ROWS = (0, 1, 63, 64, 65, 257, 1000)


@pytest.fixture(scope='module')
def ctx():
    c = ccdgpu.Context(0)
    yield c
    c.close()


def _x(n_features, n=1000, seed=11):
    return np.random.default_rng(seed).normal(size=(n, n_features))


def _forest(arrays):
    return Forest.from_arrays(*arrays.args())


def _assert_exact(ctx, forest, x, ref=None):
    ref = forest_util.walk(forest, x) if ref is None else ref
    ctx.set_forest(forest)
    got = ctx.classify(x)
    assert got.dtype == np.float32 and got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)
    return ref


@pytest.mark.parametrize('n_features', [1, 33, 64])
@pytest.mark.parametrize('n_classes', [1, 2, 9, 32])
@pytest.mark.parametrize('n_trees', [1, 7, 500])
def test_exact_against_the_walk(ctx, n_trees, n_classes, n_features):
    """Every row count around the wave and block sizes, every accumulator width, both block
    shapes (up to 35 features / more) and a forest of many LDS chunks (500 trees)."""
    depth = 5 if n_trees == 500 else 8
    f = _forest(forest_util.random_forest(1000 * n_trees + 10 * n_classes + n_features, n_trees, depth, n_features, n_classes))
    x = _x(n_features)
    ref = forest_util.walk(f, x)
    ctx.set_forest(f)
    for n in N_ROWS:
        got = ctx.classify(x[:n])
        assert got.shape == (n, n_classes) and got.dtype == np.float32
        np.testing.assert_array_equal(got, ref[:n], err_msg='n_rows %d' % n)


def test_single_leaf_trees(ctx):
    f = _forest(forest_util.random_forest(4, 5, 0, 33, 9))
    assert f.n_nodes == 5 and f.max_depth == 0
    _assert_exact(ctx, f, _x(33))


def test_trees_larger_than_lds(ctx):
    """Three complete depth-14 trees (32767 nodes each, 512 KiB of nodes alone): walked from
    global memory."""
    f = _forest(forest_util.random_forest(14, 3, 14, 33, 9, p_leaf=0.0))
    assert f.n_nodes == 3 * 32767 and f.max_depth == 14
    _assert_exact(ctx, f, _x(33))


def test_unbounded_sklearn_forest(ctx):
    """64 fully grown trees on 4000 samples of noise: about 180 k nodes."""
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.default_rng(8)
    xt = rng.normal(size=(4000, 33)).astype(np.float32)
    rf = RandomForestClassifier(n_estimators=64, random_state=1, n_jobs=16).fit(xt, rng.integers(0, 9, 4000))
    f = Forest.from_sklearn(rf)
    assert f.n_nodes > 100000 and f.n_classes == 9
    _assert_exact(ctx, f, _x(33).astype(np.float32))


def test_branch_edges(ctx):
    """x == threshold goes left, NaN goes right, +-inf compare as numbers."""
    x = _x(33, seed=12)
    one = Forest.from_arrays(root=[0], feature=[4, -1, -1], threshold=[x[0, 4], 0, 0], left=[1, -1, -1], right=[2, -1, -1],
                             value=[[0, 0], [1, 0], [0, 1]], n_features=33)
    probe = np.tile(x[0], (5, 1))
    probe[1, 4], probe[2, 4], probe[3, 4], probe[4, 4] = np.nan, np.inf, -np.inf, np.nextafter(x[0, 4], np.inf)
    ctx.set_forest(one)
    np.testing.assert_array_equal(ctx.classify(probe), np.float32([[1, 0], [0, 1], [0, 1], [1, 0], [0, 1]]))
    # thresholds taken from the rows themselves: most rows meet a threshold they equal
    f = _forest(forest_util.random_forest(21, 40, 8, 33, 9, rows=x))
    hits = np.isin(x, f.threshold[f.feature >= 0]).any(axis=1).sum()
    assert hits > 500
    _assert_exact(ctx, f, x)
    y = x.copy()
    rng = np.random.default_rng(13)
    for v in (np.nan, np.inf, -np.inf):
        y[rng.integers(0, 1000, 400), rng.integers(0, 33, 400)] = v
    y[7] = np.nan
    _assert_exact(ctx, f, y)


def test_batch_independence(ctx):
    f = _forest(forest_util.random_forest(31, 7, 8, 33, 9))
    x = _x(33, seed=14)
    ctx.set_forest(f)
    whole = ctx.classify(x)
    for step in (1, 64, 257):
        parts = np.concatenate([ctx.classify(x[i:i + step]) for i in range(0, 1000, step)])
        assert parts.tobytes() == whole.tobytes(), step


def test_sklearn_reference_shape(ctx):
    """The reference's forest shape: 500 trees of depth 5, 9 classes, 33 features (the LDS
    path: at most 63 nodes a tree).  predict_proba is the mean of the trees' distributions in an
    order of sklearn's choosing: equal to rfrawp / 500 within one float32 rounding."""
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.default_rng(9)
    xt = rng.normal(size=(1500, 33)).astype(np.float32)
    yt = (np.abs(xt[:, :3]).sum(axis=1) * 2).astype(np.int64) % 9
    rf = RandomForestClassifier(n_estimators=500, max_depth=5, random_state=2, n_jobs=16).fit(xt, yt)
    f = Forest.from_sklearn(rf)
    assert (f.n_trees, f.n_classes, f.n_features) == (500, 9, 33) and f.max_depth <= 5
    x = rng.normal(size=(1000, 33)).astype(np.float32)
    ref = _assert_exact(ctx, f, x)
    np.testing.assert_allclose(ctx.classify(x) / 500, rf.predict_proba(x), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ref / 500, rf.predict_proba(x), rtol=1e-6, atol=1e-6)


def _aux_at(cx, n_pix, seed):
    """tests/test_gpu_features.py's aux recipe for a chip at (cx, CY)."""
    import pyarrow as pa
    from test_gpu_features import CX, _aux
    t = _aux(n_pix, seed=seed)
    shift = pa.scalar(cx - CX, pa.int32())
    for name in ('cx', 'px'):
        i = t.schema.get_field_index(name)
        t = t.set_column(i, name, pc.add(t[name], shift))
    return t


def test_chained_path_matches_predictions(ctx):
    """classify_chips_tables (detection, then the rows gathered and classified on the device)
    against predictions() over the same segment tables (Arrow join, features.matrix, the
    host-matrix path): the chip of tests/test_gpu_features.py with one all-fill pixel, and a
    second chip of the same dates so that the batch has two."""
    import pyarrow as pa
    from ccdc import chipmunk, pyccd
    from ccdgpu import synth
    from test_gpu_features import CX, CY
    n_pix = 300
    locs = [(CX, CY), (CX + 3000, CY)]
    chips, aux, aux5 = [], {}, {}
    for i, (cx, cy) in enumerate(locs):
        d, s, q = synth.chip(synth.config(5), 4, 300 * i, n_pix)
        order = np.argsort(d)[::-1]
        d, s, q = d[order], s[:, :, order].copy(), q[:, order].copy()
        if i == 0:
            q[17, :] = 1  # fill: no clear observation, no model -> pyccd.default's row
            s[:, 17, :] = -9999
        chips += chipmunk.chip_response(cx, cy, d, s, q)
        aux[cx, cy] = _aux_at(cx, n_pix, seed=3 + i)
        aux5[cx, cy] = np.stack([features._first(aux[cx, cy][k]) for k in ('dem', 'aspect', 'slope', 'mpw', 'posidex')], axis=1)
    plain = dict(pyccd.detect_chips_tables(chips, context=ctx))
    assert list(plain) == locs
    plain_all = pa.concat_tables([plain[k]['segment'] for k in locs])
    aux_all = pa.concat_tables([aux[k] for k in locs])
    has_model = pc.is_valid(plain_all['chprob']).to_numpy(zero_copy_only=False)
    assert (~has_model).sum() >= 1 and plain_all.num_rows > 2 * n_pix
    m = features.matrix(features.independent(features.join({'aux': aux_all, 'ccd': plain_all})))
    forest = _forest(forest_util.random_forest(41, 50, 6, 33, 9, rows=m[has_model]))

    got_tabs = randomforest.classify_chips_tables(chips, lambda cx, cy: aux5[cx, cy], forest, context=ctx)
    assert [k for k, _ in got_tabs] == locs
    seg = pa.concat_tables([t['segment'] for _, t in got_tabs])
    assert seg.num_rows == plain_all.num_rows
    assert seg.drop_columns(['rfrawp']).equals(plain_all.drop_columns(['rfrawp']))
    for (k, t) in got_tabs:
        assert t['segment'].num_rows == plain[k]['segment'].num_rows
        assert t['pixel'].equals(plain[k]['pixel']) and t['chip'].equals(plain[k]['chip'])
    got = seg['rfrawp'].to_pylist()
    assert [g is None for g in got] == (~has_model).tolist()
    # a short buffer: CCDGPU_EINVAL with the row count set (the batch is still the last run)
    both = np.concatenate([aux5[k] for k in locs])
    with pytest.raises(ccdgpu.CcdGpuError) as e:
        ctx.classify_rows(both, rows_cap=plain_all.num_rows - 1)
    assert e.value.code == abi.E_INVAL and ctx.forest_rows == plain_all.num_rows
    raw = ctx.classify_rows(both)
    assert raw.shape == (plain_all.num_rows, 9)
    assert np.isnan(raw[~has_model]).all() and not np.isnan(raw[has_model]).any()

    pred = randomforest.predictions(aux_all, plain_all, forest, context=ctx)
    assert pred.num_rows == has_model.sum()
    joined = randomforest.join(plain_all, pred)
    assert joined.drop_columns(['rfrawp']).equals(plain_all.filter(has_model).drop_columns(['rfrawp']))
    want = np.float32(joined['rfrawp'].to_pylist())
    np.testing.assert_array_equal(np.float32([g for g in got if g is not None]), want)
    np.testing.assert_array_equal(raw[has_model], want)
    np.testing.assert_array_equal(want, forest_util.walk(forest, m[has_model]))


def test_more_rows_than_one_slab(ctx):
    """The host-matrix path uploads 2^20 rows at a time: a matrix that crosses the slab."""
    f = _forest(forest_util.random_forest(61, 3, 4, 1, 2))
    x = _x(1, n=(1 << 20) + 65, seed=15)
    _assert_exact(ctx, f, x)


def test_lifecycle(ctx):
    fresh = ccdgpu.Context(0)
    try:
        x = _x(33)
        with pytest.raises(ccdgpu.CcdGpuError):
            fresh.classify(x)
        out = np.zeros((4, 9), dtype=np.float32)
        secs = ctypes.c_double(0.0)
        rc = ccdgpu.lib().ccdgpu_classify(fresh._ctx, x.ctypes.data, 4, out.ctypes.data, ctypes.byref(secs))
        assert rc == abi.E_INVAL and 'no forest' in ccdgpu.last_error()
        a = _forest(forest_util.random_forest(51, 7, 6, 33, 9))
        b = _forest(forest_util.random_forest(52, 3, 4, 33, 2))
        ra = _assert_exact(fresh, a, x)
        rb = _assert_exact(fresh, b, x)
        assert ra.shape != rb.shape
        _assert_exact(fresh, a, x, ra)
        bad, keep = abi.forest_struct([0], [0, -1, -1], [0.0, 0, 0], [0, -1, -1], [2, -1, -1], np.ones((3, 2)), 33)
        with pytest.raises(ValueError, match='not greater'):
            fresh.set_forest(bad)
        np.testing.assert_array_equal(fresh.classify(x), ra)  # a rejected forest leaves the old one
        fresh.clear_forest()
        with pytest.raises(ccdgpu.CcdGpuError):
            fresh.classify(x)
        (d, s, q), params, ref = golden_util.load('ref_ard12')
        problems, max_rel = parity_util.compare(fresh.detect_batch(d, s, q, params=params), ref)
        assert not problems and max_rel < parity_util.RTOL
    finally:
        fresh.close()
