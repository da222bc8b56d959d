"""The random forest's bin edges on the device (ccd_splits.hip through Context.find_splits) against
ccdc.randomforest.find_splits on the host: every comparison is array_equal, feature by feature.

Shapes are the smallest at which each part can go wrong:
  rows      0 (no launch), 1 and 2 (no boundary, one), 63 / 64 / 65 (a wave of the walk and of the
            scatter's ballots, one lane short and one over), TILE - 1 / TILE / TILE + 1 (the sort's tile of
            CCD_SPLITS_TILE = 4096 keys: a second block with one key), 2 * TILE + 1000 (three tiles, the last
            one partial: the scan over tiles and the boundary offsets run over more than one entry),
            2^20 + 3 (a second upload slab, three rows long; 257 tiles: the scans take more than one chunk
            of 64 tiles per wave, and with continuous values the walk searches a million boundaries)
  max_bins  2 (one edge), 3, 32 (the default) and 64 (63 edges: every lane of the walk but one)
  features  1, 33 (the reference's) and 64 (the most), in groups of 1, 2 and all at once
  columns   tests/splits_util.py ``kinds``, each between ordinary columns, at 5000 rows (two tiles)
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ccdgpu
import forest_util
import splits_util as su
import train_util as tu
from ccdgpu import abi
from ccdc import randomforest
from ccdc.randomforest import Forest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r'#define CCD_SPLITS_TILE (\d+)',
                     open(os.path.join(ROOT, 'lcmap-firebird_amd', 'csrc', 'ccd_splits.h')).read()).group(1))


@pytest.fixture(scope='module')
def ctx():
    c = ccdgpu.Context(0)
    yield c
    c.close()


def _same(ctx, x, max_bins, ref=None):
    got = ctx.find_splits(x, max_bins)
    ref = su.host(x, max_bins) if ref is None else ref
    assert len(got) == len(ref) == x.shape[1]
    for f, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == np.float64 and a.flags['C_CONTIGUOUS'] and np.array_equal(a, b), (f, a, b)
    return got


def _mixed(seed, n, nf):
    """Columns by turns continuous, tied (a skew of integers) and coarsely rounded, of both signs."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, nf))
    x[:, 1::3] = np.floor(40.0 * rng.exponential(size=x[:, 1::3].shape))
    x[:, 2::3] = np.round(x[:, 2::3], 1)
    return x


def test_tile_is_the_one_the_shapes_assume():
    assert TILE == 4096


@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1000])
def test_row_counts(ctx, n):
    x = _mixed(n, n, 3)
    for max_bins in (2, 32):
        got = _same(ctx, x, max_bins)
        if n <= 1:
            assert [e.shape for e in got] == [(0,)] * 3


def test_rows_beyond_one_upload_slab(ctx):
    """2^20 + 3 rows of 2 features: the last three rows, alone in the second slab, hold the column's
    three largest values and, in the tied column, a value of their own."""
    n = (1 << 20) + 3
    rng = np.random.default_rng(41)
    x = np.empty((n, 2))
    x[:, 0] = rng.normal(size=n)
    x[:, 1] = rng.integers(0, 50, size=n)
    x[-3:, 0] = (7.0, 8.0, 9.0)
    x[-3:, 1] = 77.0
    got = _same(ctx, x, 64)
    assert got[0].shape == (63,) and got[1].shape == (50,) and got[1][-1] == (49.0 + 77.0) / 2.0


@pytest.mark.parametrize('max_bins', [2, 3, 32, 64])
def test_column_kinds_between_ordinary_columns(ctx, max_bins):
    n = 5000
    cols = su.kinds(n, max_bins, seed=max_bins)
    rng = np.random.default_rng(100 + max_bins)
    names, stack = [], []
    for name, c in cols.items():
        names += ['ordinary before ' + name, name]
        stack += [rng.normal(size=n), c]
    x = np.stack(stack, axis=1)
    assert x.shape[1] <= 64
    ref = su.host(x, max_bins)
    got = ctx.find_splits(x, max_bins)
    for name, a, b in zip(names, got, ref):
        assert np.array_equal(a, b), (name, a, b)
    by = dict(zip(names, got))
    assert by['constant'].shape == (0,) and by['distinct_+0'].shape == (max_bins - 1,)
    if max_bins >= 32:  # (six and seven distinct values: every boundary's midpoint)
        assert np.isneginf(by['huge_both_sides'][0]) and np.isposinf(by['huge_both_sides'][-1])
        assert by['neighbouring_doubles'].shape[0] < 5
        assert by['both_signs_and_zeros'].tolist() == [-2.5, -1.5, -0.5, 0.5, 1.5, 2.5]


def test_one_value_spans_several_targets(ctx):
    """The hand case of tests/test_randomforest_train.py: counts 10, 1, 1, 1, 1, 1, 1 at max_bins 4."""
    x = np.stack([np.arange(16.0), np.asarray(su.HAND), -np.arange(16.0)], axis=1)
    got = _same(ctx, x, 4)
    assert got[1].tolist() == [0.5, 1.5, 2.5]


@pytest.mark.parametrize('nf', [1, 33, 64])
def test_feature_counts_and_groups(ctx, monkeypatch, nf):
    x = _mixed(nf, 1500, nf)
    x[:, nf // 2] = 3.5  # a constant column inside a group
    ref = su.host(x, 32)
    _same(ctx, x, 32, ref)
    for group in ('1', '2'):  # groups of one feature; of two, the last one of one feature when nf is odd
        monkeypatch.setenv('CCDGPU_SPLITS_GROUP_FEATURES', group)
        _same(ctx, x, 32, ref)
    monkeypatch.delenv('CCDGPU_SPLITS_GROUP_FEATURES')
    _same(ctx, x, 32, ref)


def test_row_order_does_not_matter(ctx):
    x = _mixed(9, TILE + 500, 6)
    got = _same(ctx, x, 32)
    again = ctx.find_splits(x[np.random.default_rng(1).permutation(x.shape[0])], 32)
    assert su.same(got, again)
    assert su.same(got, ctx.find_splits(np.sort(x, axis=0)[::-1], 32))  # every column descending


def test_through_randomforest_find_splits_and_the_c_abi(ctx):
    x = _mixed(12, 700, 5)
    ref = su.host(x, 16)
    assert su.same(randomforest.find_splits(x, 16, context=ctx), ref)
    assert ctx.splits_seconds > 0.0
    assert su.same(randomforest.find_splits(x.tolist(), 16, context=ctx), ref)  # an array-like
    # the C call itself: zeros behind every feature's edges, kernel_seconds may be NULL
    edges = np.full((5, abi.TRAIN_MAX_EDGES), -7.0)
    n_edges = np.full(5, -7, dtype=np.int32)
    rc = ccdgpu.lib().ccdgpu_forest_find_splits(ctx._ctx, x.ctypes.data, x.shape[0], 5, 16, edges.ctypes.data,
                                                n_edges.ctypes.data, None)
    assert rc == 0 and n_edges.tolist() == [e.shape[0] for e in ref]
    for f in range(5):
        assert np.array_equal(edges[f, :n_edges[f]], ref[f]) and np.all(edges[f, n_edges[f]:] == 0.0)
    rc = ccdgpu.lib().ccdgpu_forest_find_splits(ctx._ctx, x.ctypes.data, x.shape[0], 5, 16, None, n_edges.ctypes.data, None)
    assert rc == abi.E_INVAL and 'edges is NULL' in ccdgpu.last_error()
    rc = ccdgpu.lib().ccdgpu_forest_find_splits(ctx._ctx, x.ctypes.data, x.shape[0], 5, 16, edges.ctypes.data, None, None)
    assert rc == abi.E_INVAL and 'n_edges is NULL' in ccdgpu.last_error()


def test_refusals_name_the_row_and_feature(ctx):
    x = _mixed(13, 300, 4)
    ctx.find_splits(x, 32)
    before = ctx.splits_seconds
    for bad in (np.nan, np.inf, -np.inf):
        x2 = x.copy()
        x2[217, 3] = bad
        with pytest.raises(ValueError, match=r'splits: x\[217\]\[3\] is not finite'):
            ctx.find_splits(x2, 32)
        with pytest.raises(ValueError, match=r'splits: x\[217\]\[3\] is not finite'):
            randomforest.find_splits(x2, 32, context=ctx)
    for max_bins in (1, 65):
        with pytest.raises(ValueError, match='max_bins must be in'):
            ctx.find_splits(x, max_bins)
    with pytest.raises(ValueError, match='n_features'):
        ctx.find_splits(np.zeros((4, 65)), 32)
    with pytest.raises(ValueError, match='n_rows'):
        ctx.find_splits(np.zeros(4), 32)
    assert ctx.splits_seconds == before  # nothing ran
    rc = ccdgpu.lib().ccdgpu_forest_find_splits(None, x.ctypes.data, 300, 4, 32, None, None, None)
    assert rc == abi.E_INVAL


def test_forests_of_the_context_are_untouched(ctx):
    x, y = _mixed(17, 400, 33), (np.arange(400) % 5).astype(np.int32)
    mine = forest_util.random_forest(5, 6, 4, 33, 9)
    ctx.set_forest(Forest.from_arrays(*mine.args()))
    raw = ctx.classify(x)
    edges = su.host(x, 16)
    trained = ctx.train_forest(x, y, edges, n_classes=5, n_trees=3, max_depth=3, seed=2)
    _same(ctx, x, 16, edges)
    assert np.array_equal(ctx.classify(x), raw)
    nt, nn = ctypes.c_int32(0), ctypes.c_int32(0)
    assert ccdgpu.lib().ccdgpu_trained_size(ctx._ctx, ctypes.byref(nt), ctypes.byref(nn)) == 0
    assert (nt.value, nn.value) == (trained.n_trees, trained.n_nodes)
    ctx.clear_forest()


def test_training_with_device_splits_equals_host_splits(ctx):
    """ccdc.randomforest.train over features.dataframe of a chip the device detected (the table of
    tests/test_gpu_randomforest_train.py): splits='device' gives the forest of splits='host', all six
    arrays and the counts."""
    from ccdc import chipmunk, features, pyccd
    from ccdgpu import synth
    from test_gpu_features import CX, CY, _aux
    n_pix = 100
    d, s, q = synth.chip(synth.config(5), 4, 0, n_pix)
    order = np.argsort(d)[::-1]
    d, s, q = d[order], s[:, :, order], q[:, order]
    (key, t), = pyccd.detect_chips_tables(chipmunk.chip_response(CX, CY, d, s, q))
    table = features.dataframe(_aux(n_pix), t['segment'])
    par = dict(n_trees=6, max_depth=4, max_bins=16, seed=3, context=ctx)
    on_host = randomforest.train(table, splits='host', **par)
    on_device = randomforest.train(table, splits='device', **par)
    assert tu.equal(on_device, on_host) == [] and np.array_equal(on_device.counts, on_host.counts)
    assert (on_device.rows_trained, on_device.rows_dropped) == (on_host.rows_trained, on_host.rows_dropped)
    assert tu.equal(randomforest.train(table, **par), on_host) == []  # the default is the host's
    m = features.matrix(table)
    keep = np.all(np.isfinite(m), axis=1) & np.isfinite(np.asarray(table['label'].to_pylist(), dtype=np.float64))
    _same(ctx, np.ascontiguousarray(m[keep]), 16)
