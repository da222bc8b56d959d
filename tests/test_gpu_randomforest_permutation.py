"""The out-of-bag permutation counts on the device (ccd_forest_permutation in ccd_forest.hip through
Context.forest_permutation) against the numpy restatement of the rule (tests/permutation_util.py, which
walks every row for every feature and so knows nothing of the kernel's path shortcut): every comparison
is array_equal on all four arrays.  The kernel cases use generated forests at the smallest shapes at
which each path runs: both launch shapes around their block sizes, several LDS chunks, a tree walked
from global memory, a second upload slab."""
import ctypes

import numpy as np
import pytest

import ccdgpu
import forest_util
import oob_util
import permutation_util as pu
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


def _labels(seed, n, nc):
    return np.random.default_rng(seed + 1000).integers(0, nc, size=n).astype(np.int32)


def _identities(ctx, f, x, seed, got):
    """What holds for any forest and rows (the forest is the context's)."""
    oob_rows, correct, lost, gained = got
    assert oob_rows.sum() == ctx.forest_oob(x, seed)[1].sum()
    assert np.all(correct <= oob_rows) and np.all(correct >= 0)
    assert np.all(lost >= 0) and np.all(lost <= correct[:, None, :])
    assert np.all(gained >= 0) and np.all(gained <= (oob_rows - correct)[:, None, :])
    for t, root in enumerate(np.asarray(f.root).tolist()):
        never = sorted(set(range(f.n_features)) - pu.tested(f, root))
        assert not lost[t, never].any() and not gained[t, never].any()


def _same(ctx, f, x, y, seed, perm_seed=0):
    ctx.set_forest(Forest.from_arrays(*f.args()))
    got = ctx.forest_permutation(x, y, seed, perm_seed)
    ref = pu.counts(f, x, y, seed, perm_seed)
    nt, nc = np.asarray(f.root).shape[0], np.asarray(f.value).shape[1]
    for name, a, b in zip(('oob_rows', 'correct', 'lost', 'gained'), got, ref):
        assert a.dtype == np.int64 and a.shape == b.shape == ((nt, nc) if a.ndim == 2 else (nt, f.n_features, nc)), name
        assert np.array_equal(a, b), name
    _identities(ctx, f, x, seed, got)
    return got


@pytest.mark.parametrize('n_rows,nf', [(1, 5), (2, 5), (63, 5), (64, 5), (65, 5), (511, 5), (512, 5), (513, 5), (1000, 5),
                                       (255, 64), (256, 64), (257, 64)])
def test_row_counts(ctx, n_rows, nf):
    assert ccdgpu.lib().ccdk_forest_threads(nf) == (512 if nf == 5 else 256)
    x = _rows(n_rows, n_rows, nf)
    _same(ctx, forest_util.random_forest(3, 3, 7, nf, 3, rows=x), x, _labels(n_rows, n_rows, 3), seed=n_rows, perm_seed=7)


@pytest.mark.parametrize('n_classes', [1, 2, 3, 4, 5, 9, 10, 16, 17, 32])
def test_class_counts(ctx, n_classes):
    x = _rows(n_classes, 130, 6)
    got = _same(ctx, forest_util.random_forest(n_classes, 9, 4, 6, n_classes), x, _labels(n_classes, 130, n_classes), seed=4)
    if n_classes == 1:  # every vote is right and stays right
        assert np.array_equal(got[0], got[1]) and not got[2].any() and not got[3].any()


def test_several_chunks(ctx):
    f = forest_util.random_forest(11, 70, 5, 33, 9, p_leaf=0.0)
    cap = ccdgpu.lib().ccdk_forest_chunk_cap(33)
    assert 70 * (63 * 16 + 32 * 9 * 8) > 2 * cap  # the forest's blobs need more than two chunks
    got = _same(ctx, f, _rows(12, 700, 33), _labels(12, 700, 9), seed=6, perm_seed=3)
    assert got[2].any() and got[3].any()


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
    got = _same(ctx, f, _rows(16, 700, 33), _labels(16, 700, 9), seed=8, perm_seed=5)
    assert got[2][1].any() and got[3][1].any()  # the big tree's votes change


def test_one_forest_three_walks(ctx):
    """The classification, the out-of-bag walk and the permutation counts share one chunk loop: one forest
    whose trees need several LDS chunks on either side of a tree that no chunk holds, over 513 rows (a
    second block of one row), through all three against their restatements."""
    nf, nc, n = 5, 3, 513
    cap = ccdgpu.lib().ccdk_forest_chunk_cap(nf)
    small, big = 63 * 16 + 32 * nc * 8, 1023 * 16 + 512 * nc * 8  # the blobs of complete trees of depth 5 and 9
    assert ccdgpu.lib().ccdk_forest_threads(nf) == 512 and big > cap and 14 * small > cap
    f = forest_util.concatenated([forest_util.random_forest(61, 14, 5, nf, nc, p_leaf=0.0),
                                  forest_util.random_forest(62, 1, 9, nf, nc, p_leaf=0.0),
                                  forest_util.random_forest(63, 14, 5, nf, nc, p_leaf=0.0)])
    assert f.root.shape[0] == 29 and f.feature.shape[0] == 28 * 63 + 1023
    x, y = _rows(64, n, nf), _labels(64, n, nc)
    got = _same(ctx, f, x, y, seed=9, perm_seed=2)
    assert got[2][14].any() and got[3][14].any() and got[2][28].any()  # the big tree and the last chunk count
    assert np.array_equal(ctx.classify(x), forest_util.walk(f, x))
    raw, scored = ctx.forest_oob(x, 9)
    ref_raw, ref_scored = oob_util.oob(f, x, 9)
    assert np.array_equal(raw, ref_raw) and np.array_equal(scored, ref_scored)


def test_a_stump_on_the_last_of_64_features(ctx):
    """Bit 63 of the path mask.  A row's label is its side of the stump, so every vote is right; shuffling
    column 63 loses exactly the out-of-bag rows whose donor sits on the other side."""
    n = 200
    y = _labels(39, n, 2)
    x = np.zeros((n, 64))
    x[:, 63] = y
    f = forest_util.Arrays([0], [63, -1, -1], [0.5, 0.0, 0.0], [1, -1, -1], [2, -1, -1], [[0.5, 0.5], [1, 0], [0, 1]], 64)
    oob_rows, correct, lost, gained = _same(ctx, f, x, y, seed=2, perm_seed=9)
    out = oob_util.out_of_bag(2, 0, 0, n)
    donor = pu.donors(9, 0, 63, n).astype(np.int64)
    flipped = out & (y[donor] != y)
    assert flipped.any() and not flipped[out].all()
    assert np.array_equal(oob_rows, correct) and oob_rows[0].tolist() == np.bincount(y[out], minlength=2).tolist()
    assert lost[0, 63].tolist() == np.bincount(y[flipped], minlength=2).tolist()
    assert not lost[0, :63].any() and not gained.any()


def test_a_feature_twice_on_a_path_counts_once(ctx):
    """x[1] <= 0.5 ? (x[1] <= -0.5 ? class 0 : class 1) : class 2: the left path tests feature 1 twice."""
    f = forest_util.Arrays([0], [1, 1, -1, -1, -1], [0.5, -0.5, 0, 0, 0], [1, 2, -1, -1, -1], [4, 3, -1, -1, -1],
                           [[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], 3)
    n = 300
    x = _rows(41, n, 3)
    y = np.where(x[:, 1] <= -0.5, 0, np.where(x[:, 1] <= 0.5, 1, 2)).astype(np.int32)
    oob_rows, correct, lost, gained = _same(ctx, f, x, y, seed=5, perm_seed=1)
    out = oob_util.out_of_bag(5, 0, 0, n)
    donor = pu.donors(1, 0, 1, n).astype(np.int64)
    assert np.array_equal(oob_rows, correct)
    assert lost[0, 1].tolist() == np.bincount(y[out & (y[donor] != y)], minlength=3).tolist()  # once per row, not twice
    assert lost[0, 1].sum() > 0 and not lost[0, [0, 2]].any() and not gained.any()


def test_tied_leaves_vote_for_the_lower_class(ctx):
    """Leaves [0.5, 0.5, 0] (vote 0) and [0.2, 0.4, 0.4] (vote 1): the comparisons are on the doubles as they are."""
    f = forest_util.Arrays([0], [0, -1, -1], [0.0, 0.0, 0.0], [1, -1, -1], [2, -1, -1],
                           [[0, 0, 0], [0.5, 0.5, 0.0], [0.2, 0.4, 0.4]], 2)
    n = 400
    x = _rows(43, n, 2)
    y = _labels(43, n, 3)
    oob_rows, correct, lost, gained = _same(ctx, f, x, y, seed=6, perm_seed=2)
    out = oob_util.out_of_bag(6, 0, 0, n)
    vote = np.where(x[:, 0] <= 0.0, 0, 1)
    assert correct[0].tolist() == np.bincount(y[out & (vote == y)], minlength=3).tolist()
    assert correct[0, 2] == 0 and gained[0, :, 2].sum() == 0 and oob_rows[0, 2] > 0  # no leaf ever votes 2


def test_nan_in_a_row_and_in_its_donors(ctx):
    x = _rows(29, 100, 4)
    x[::3, 1] = np.nan
    x[5] = np.nan
    f = forest_util.random_forest(30, 6, 3, 4, 3, p_leaf=0.0)
    _same(ctx, f, x, _labels(29, 100, 3), seed=12, perm_seed=4)
    # a stump on the column with the NaNs: a NaN of its own, or a donor's, sends the row right
    one = forest_util.Arrays([0], [1, -1, -1], [0.0, 0.0, 0.0], [1, -1, -1], [2, -1, -1], [[0, 0], [1, 0], [0, 1]], 4)
    with np.errstate(invalid='ignore'):
        y = np.where(x[:, 1] <= 0.0, 0, 1).astype(np.int32)
    oob_rows, correct, lost, gained = _same(ctx, one, x, y, seed=12, perm_seed=4)
    out = oob_util.out_of_bag(12, 0, 0, 100)
    donor = pu.donors(4, 0, 1, 100).astype(np.int64)
    to_nan = out & np.isnan(x[donor, 1]) & (y == 0)
    assert to_nan.any() and np.array_equal(oob_rows, correct) and lost[0, 1, 0] >= to_nan.sum()


@pytest.mark.parametrize('seed', [0, 1, 2 ** 63 + 5, 2 ** 64 - 1])
def test_seeds(ctx, seed):
    x = _rows(21, 300, 5)
    f = forest_util.random_forest(22, 12, 4, 5, 4)
    y = _labels(21, 300, 4)
    _same(ctx, f, x, y, seed=seed, perm_seed=3)
    _same(ctx, f, x, y, seed=3, perm_seed=seed)


def test_rows_beyond_one_upload_slab(ctx):
    """2^20 + 3 rows: the matrix goes up in two slabs into one buffer, and donors cross between them."""
    n = (1 << 20) + 3
    x = _rows(27, n, 1)
    f = forest_util.random_forest(28, 3, 1, 1, 2, p_leaf=0.0)
    got = _same(ctx, f, x, _labels(27, n, 2), seed=11, perm_seed=6)
    assert got[2].any() and got[3].any() and ctx.permutation_seconds > 0.0


def test_a_second_call_returns_the_same_arrays(ctx):
    x = _rows(51, 700, 7)
    y = _labels(51, 700, 5)
    f = forest_util.random_forest(52, 10, 5, 7, 5)
    first = _same(ctx, f, x, y, seed=14, perm_seed=8)
    again = ctx.forest_permutation(x, y, 14, 8)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))  # the counters are zeroed by every call
    other = ctx.forest_permutation(x, y, 14, 9)
    assert np.array_equal(other[0], first[0]) and np.array_equal(other[1], first[1])  # the bags and votes are the same
    assert not np.array_equal(other[2], first[2])                                     # the shuffles are not


def _size(L, ctx):
    nt, nn = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.ccdgpu_trained_size(ctx._ctx, ctypes.byref(nt), ctypes.byref(nn)) == 0
    return nt.value, nn.value


def test_state_is_left_alone_and_refusals(ctx):
    x = _rows(35, 300, 33)
    y = (np.arange(300) % 4).astype(np.int32)
    ctx.train_forest(x, y, randomforest.find_splits(x, 8), n_classes=4, n_trees=3, max_depth=3, seed=1)
    L = ccdgpu.lib()
    before = _size(L, ctx)
    f = forest_util.random_forest(36, 6, 4, 33, 9)
    _same(ctx, f, x, y, seed=13)
    assert np.array_equal(ctx.classify(x), forest_util.walk(f, x))
    raw, n = ctx.forest_oob(x, 13)
    ref_raw, ref_n = oob_util.oob(f, x, 13)
    assert np.array_equal(raw, ref_raw) and np.array_equal(n, ref_n)
    assert _size(L, ctx) == before
    # refusals with a forest set: a wrong feature count, a bad label with its index, no rows
    with pytest.raises(ValueError):
        ctx.forest_permutation(np.zeros((3, 5)), [0, 1, 2], 1)
    bad = y.copy()
    bad[17] = 9
    with pytest.raises(ccdgpu.CcdGpuError, match=r'permutation: labels\[17\] = 9') as err:
        ctx.forest_permutation(x, bad, 13)
    assert err.value.code == ccdgpu.abi.E_INVAL
    bad[17] = -1
    with pytest.raises(ccdgpu.CcdGpuError, match=r'permutation: labels\[17\] = -1'):
        ctx.forest_permutation(x, bad, 13)
    none = ctx.forest_permutation(np.zeros((0, 33)), np.zeros(0, np.int32), 13)
    assert [a.shape for a in none] == [(6, 9), (6, 9), (6, 33, 9), (6, 33, 9)]
    assert all(a.dtype == np.int64 and not a.any() for a in none)
    # without a forest: the binding's refusal, then the library's
    ctx.clear_forest()
    with pytest.raises(ccdgpu.CcdGpuError, match='no forest set') as err:
        ctx.forest_permutation(x, y, 13)
    assert err.value.code == ccdgpu.abi.E_INVAL
    ctx._forest_shape = (33, 9)
    try:
        with pytest.raises(ccdgpu.CcdGpuError, match='no forest set') as err:
            ctx.forest_permutation(x, y, 13)
        assert err.value.code == ccdgpu.abi.E_INVAL
    finally:
        ctx._forest_shape = None


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid='ignore'):
        return np.where(same, 0.0, np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))


def _agrees(s, x, y, forest, seed, perm_seed):
    """The counts equal the restatement's, and the host floats its plain loop within 4 ulps."""
    ref = pu.counts(forest, x, y, seed, perm_seed)
    for name, b in zip(('oob_rows', 'correct', 'lost', 'gained'), ref):
        assert np.array_equal(getattr(s, name), b), name
    imp, std, per_class, used = pu.importances(ref[0], ref[2], ref[3])
    assert s.trees_used == used
    assert _ulps(s.importances, imp).max() <= 4 and _ulps(s.importances_std, std).max() <= 4
    assert _ulps(s.class_importances, per_class).max() <= 4


def test_importances_of_the_perfect_case(ctx):
    """train_util.perfect_case, label = x[:, 7] // 3 over four classes.  With every feature offered at every
    node each tree splits on feature 7 only, so only its shuffle can change a vote, and only for the worse:
    about 3/4 of the votes are lost (the restatement: lost.sum() 849, importances[7] 0.76272).  With sqrt(33)
    features per node other features are split on where 7 is not offered, and 7 still stands out (the
    restatement: 0.2091 against 0.0050 for the runner-up)."""
    x, y, edges = tu.perfect_case()
    forest = ctx.train_forest(x, y, edges, n_trees=5, max_depth=5, features_per_node='all', seed=3)
    assert set(forest.feature[forest.feature >= 0].tolist()) == {7}
    s = randomforest.permutation_importances(forest, x, y, perm_seed=11, context=ctx)
    _agrees(s, x, y, forest, 3, 11)
    _identities(ctx, forest, x, 3, (s.oob_rows, s.correct, s.lost, s.gained))
    assert not s.gained.any() and np.array_equal(s.correct, s.oob_rows)
    assert s.trees_used == 5 and np.all(np.delete(s.importances, 7) == 0.0)
    assert abs(s.importances[7] - 0.75) < 0.05 and s.lost.sum() == s.lost[:, 7].sum() > 0
    print('all: lost.sum() %d importances[7] %.5f' % (s.lost.sum(), s.importances[7]))
    forest = ctx.train_forest(x, y, edges, n_trees=20, max_depth=5, features_per_node='sqrt', seed=3)
    s = randomforest.permutation_importances(forest, x, y, perm_seed=11, context=ctx)
    _agrees(s, x, y, forest, 3, 11)
    order = np.argsort(s.importances)[::-1]
    assert order[0] == 7
    print('sqrt: importances[7] %.4f runner-up %.4f' % (s.importances[7], s.importances[order[1]]))
    ctx.clear_forest()


def test_train_with_permutation_over_the_features_dataframe(ctx):
    """ccdc.randomforest.train(dataframe, permutation=True) over features.dataframe of a chip the device
    detected: the forest is the plain one, and forest.permutation the importances over the kept rows."""
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
    assert not hasattr(plain, 'permutation')
    forest = randomforest.train(table, n_trees=6, max_depth=4, max_bins=16, seed=3, context=ctx, permutation=True, perm_seed=2)
    assert tu.equal(forest, plain) == [] and np.array_equal(forest.counts, plain.counts)
    p = forest.permutation
    _agrees(p, x, y, forest, 3, 2)
    assert p.oob_rows.shape == (6, forest.n_classes) and p.lost.shape == (6, 33, forest.n_classes)
    assert 0 < p.oob_rows.sum() and p.trees_used == 6 and forest.rows_trained == x.shape[0]
    ctx.clear_forest()
