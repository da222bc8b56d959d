"""Random-forest training, host side: the constants and the hash of the rule (include/ccdgpu.h)
against tests/train_util.py, ccdc.randomforest.find_splits on hand-written columns, every refusal of
ccdgpu_train_check through ctypes (no device needed), the reference on a case with a known tree, and
the stand-alone sanitizer program of the check.  The device comparisons are in
tests/test_gpu_randomforest_train.py."""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ccdgpu
import forest_util
import train_util as tu
from ccdgpu import abi
from ccdc import randomforest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def test_poisson_table_is_the_cdf_of_poisson_1():
    """P[k] = floor(2^32 sum_{j<=k} e^-1 / j!), k = 0 .. 12, in exact rational arithmetic (e^-1 by its
    alternating series to 60 terms: the remainder is below 1/60!), in the header, the binding and the
    reference alike; the last entry is 2^32 - 1, so the largest weight is 13."""
    lo = sum(Fraction((-1) ** k, math.factorial(k)) for k in range(60))   # 60 terms: below e^-1
    hi = lo + Fraction(1, math.factorial(60))
    table, s_lo, s_hi = [], Fraction(0), Fraction(0)
    for k in range(13):
        s_lo += lo / math.factorial(k)
        s_hi += hi / math.factorial(k)
        assert math.floor(s_lo * 2 ** 32) == math.floor(s_hi * 2 ** 32)  # (the bounds on e^-1 agree on the floor)
        table.append(math.floor(s_lo * 2 ** 32))
    assert tuple(table) == abi.TRAIN_POISSON == tuple(int(v) for v in tu.POISSON)
    assert table[-1] == 2 ** 32 - 1
    text = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    body = text[text.index('#define CCDGPU_TRAIN_POISSON '):]
    body = body[:body.index('}')]
    assert [int(v) for v in re.findall(r'(\d+)u', body)] == table
    assert int(re.search(r'#define CCDGPU_TRAIN_POISSON_N (\d+)', text).group(1)) == 13
    assert 13 * abi.TRAIN_MAX_ROWS < 2 ** 32


def test_abi_mirrors_the_header():
    text = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    body = text[text.index('typedef struct ccdgpu_train_params'):text.index('} ccdgpu_train_params;')]
    assert re.findall(r'\b(\w+);', re.sub(r'/\*.*?\*/', '', body)) == [n for n, _ in abi.TrainParams._fields_]
    assert ctypes.sizeof(abi.TrainParams) == 40
    p, q = ccdgpu.train_params(), abi.default_train_params()
    for name, _ in abi.TrainParams._fields_:
        assert getattr(p, name) == getattr(q, name), name
    assert (p.n_trees, p.max_depth, p.features_per_node, p.min_instances_per_node, p.bootstrap) == (500, 5, 0, 1, 1)
    for name, const in (('MAX_ROWS', r'\(\(int64_t\)1 << 27\)'), ('MAX_EDGES', '63'), ('MAX_DEPTH', '10')):
        assert re.search(r'#define CCDGPU_TRAIN_%s %s\n' % (name, const), text), name
    assert (abi.TRAIN_MAX_ROWS, abi.TRAIN_MAX_EDGES, abi.TRAIN_MAX_DEPTH) == (1 << 27, 63, 10)


def test_hash_draws_the_stated_feature_subsets():
    """Seed 1, 33 features, m = 6 (the sqrt subset of 33)."""
    assert tu.subset_size(33, 0) == 6
    assert tu.subset(1, 0, 1, 33, 6).tolist() == [2, 5, 15, 26, 29, 30]
    assert tu.subset(1, 0, 2, 33, 6).tolist() == [7, 8, 9, 17, 26, 31]
    assert tu.subset(1, 1, 1, 33, 6).tolist() == [14, 15, 17, 21, 22, 23]
    assert [tu.subset_size(n, 0) for n in (1, 2, 4, 5, 9, 10, 64)] == [1, 2, 2, 3, 3, 4, 8]
    assert tu.subset_size(5, 9) == 5 and tu.subset(1, 0, 1, 5, 5).tolist() == [0, 1, 2, 3, 4]


def test_weights_are_poisson_draws_of_the_hash():
    w = tu.weights(3, 5, 20000, 1)
    assert w.min() == 0 and 5 <= w.max() <= 13
    assert abs(w.mean() - 1.0) < 0.03 and abs(w.var() - 1.0) < 0.06  # (Poisson(1): 20000 draws)
    assert abs((w == 0).mean() - math.exp(-1)) < 0.015
    assert tu.weights(3, 5, 7, 0).tolist() == [1] * 7
    assert not np.array_equal(w, tu.weights(3, 6, 20000, 1)) and not np.array_equal(w, tu.weights(4, 5, 20000, 1))


def _col(values):
    return np.asarray(values, dtype=np.float64).reshape(-1, 1)


def test_find_splits_on_hand_written_columns():
    (e,) = randomforest.find_splits(_col([3.0] * 9))
    assert e.shape == (0,) and e.dtype == np.float64                       # a constant column: never split
    (e,) = randomforest.find_splits(_col([1.0, 4.0, 4.0, 1.0, 1.0]))
    assert e.tolist() == [2.5]                                              # two values: their midpoint
    (e,) = randomforest.find_splits(_col(list(range(32)) * 2), max_bins=32)
    assert e.tolist() == [i + 0.5 for i in range(31)]                       # exactly max_bins values: every midpoint
    (e,) = randomforest.find_splits(_col(range(8)), max_bins=4)
    # 8 values once each, 3 cuts, stride 2: the count below the cut is the nearest to 2, 4, 6
    assert e.tolist() == [1.5, 3.5, 5.5]
    a = 1.0
    b = np.nextafter(a, 2.0)
    c = np.nextafter(b, 2.0)
    (e,) = randomforest.find_splits(_col([a, b, c]))
    assert np.all(np.diff(e) > 0) and 1 <= e.shape[0] <= 2 and set(e.tolist()) <= {a, b, c}  # neighbouring doubles
    x = np.random.default_rng(0).normal(size=(5000, 3))
    x[:, 1] = 2.0
    es = randomforest.find_splits(x, max_bins=32)
    assert [len(v) for v in es] == [31, 0, 31]
    for f in (0, 2):
        assert np.all(np.diff(es[f]) > 0)
        per_bin = np.bincount(np.searchsorted(es[f], x[:, f], side='left'), minlength=32)
        assert per_bin.min() > 100 and per_bin.max() < 220  # count quantiles: 5000 / 32 = 156 per bin
    with pytest.raises(ValueError):
        randomforest.find_splits(_col([1.0, np.nan]))
    with pytest.raises(ValueError):
        randomforest.find_splits(_col([1.0, 2.0]), max_bins=65)


def test_find_splits_quantile_walk_by_hand():
    """The rule's walk on counts 10, 1, 1, 1, 1, 1, 1 (16 rows, max_bins 4, stride 4): at i = 1 the count
    below is 10, |10 - 4| = 6 < |11 - 4| = 7, so 0.5 is an edge and the target becomes 8; |11 - 8| = 3 <
    |12 - 8| = 4 gives 1.5, target 12; |12 - 12| = 0 < 1 gives 2.5, target 16; then |13 - 16| = 3 > 2,
    |14 - 16| = 2 > 1, |15 - 16| = 1 > 0: no more."""
    (e,) = randomforest.find_splits(_col([0] * 10 + [1, 2, 3, 4, 5, 6]), max_bins=4)
    assert e.tolist() == [0.5, 1.5, 2.5]


def _request(n_rows=6, nf=3, nc=3):
    x = np.arange(n_rows * nf, dtype=np.float64).reshape(n_rows, nf)
    y = (np.arange(n_rows) % nc).astype(np.int32)
    n_edges = np.array([2, 0, 1], dtype=np.int32)[:nf]
    edges = np.array([1.0, 2.0, 5.0])
    return x, y, edges, n_edges, ccdgpu.train_params(n_trees=3)


def _check(x, y, edges, n_edges, p, n_rows=None, nf=None, nc=3):
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = ccdgpu.lib().ccdgpu_train_check(ptr(x), ptr(y), x.shape[0] if n_rows is None else n_rows,
                                         x.shape[1] if nf is None else nf, nc, ptr(edges), ptr(n_edges),
                                         None if p is None else ctypes.byref(p))
    return rc, ccdgpu.last_error()


def test_train_check_accepts_and_refuses():
    x, y, edges, n_edges, p = _request()
    assert _check(x, y, edges, n_edges, p)[0] == 0
    assert _check(x, y, None, np.zeros(3, np.int32), p)[0] == 0  # no edges at all: nothing to read

    def refused(needle, *args, **kw):
        rc, msg = _check(*args, **kw)
        assert rc == abi.E_INVAL and needle in msg, (needle, rc, msg)

    refused('params is NULL', x, y, edges, n_edges, None)
    for i, name in enumerate(('x', 'labels', 'edges', 'n_edges')):
        args = [x, y, edges, n_edges]
        args[i] = None
        ptrs = [None if a is None else a.ctypes.data for a in args]
        rc = ccdgpu.lib().ccdgpu_train_check(ptrs[0], ptrs[1], 6, 3, 3, ptrs[2], ptrs[3], ctypes.byref(p))
        assert rc == abi.E_INVAL and '%s is NULL' % name in ccdgpu.last_error(), name
    refused('n_rows', x, y, edges, n_edges, p, n_rows=0)
    refused('n_rows', x, y, edges, n_edges, p, n_rows=(1 << 27) + 1)
    refused('n_features', x, y, edges, n_edges, p, nf=0)
    refused('n_features', x, y, edges, n_edges, p, nf=65)
    refused('n_classes', x, y, edges, n_edges, p, nc=0)
    refused('n_classes', x, y, edges, n_edges, p, nc=33)
    refused('labels[2] = 2', x, y, edges, n_edges, p, nc=2)
    y2 = y.copy()
    y2[4] = -1
    refused('labels[4] = -1', x, y2, edges, n_edges, p)
    for bad in (np.nan, np.inf, -np.inf):
        x2 = x.copy()
        x2[3, 1] = bad
        refused('x[3][1] is not finite', x2, y, edges, n_edges, p)
    refused('n_edges[1]', x, y, edges, np.array([2, 64, 1], np.int32), p)
    refused('n_edges[2]', x, y, edges, np.array([2, 0, -1], np.int32), p)
    refused('feature 0: edge 1 is not above edge 0', x, y, np.array([1.0, 1.0, 5.0]), n_edges, p)
    refused('feature 0: edge 1 is not above edge 0', x, y, np.array([2.0, 1.0, 5.0]), n_edges, p)
    refused('feature 2: edge 0 is not finite', x, y, np.array([1.0, 2.0, np.inf]), n_edges, p)
    refused('feature 0: edge 1 is not finite', x, y, np.array([1.0, np.nan, 5.0]), n_edges, p)
    for field, value in (('n_trees', 0), ('max_depth', -1), ('max_depth', 11), ('features_per_node', -1),
                         ('min_instances_per_node', 0), ('min_info_gain', -0.5), ('min_info_gain', np.nan),
                         ('bootstrap', 2)):
        q = ccdgpu.train_params(n_trees=3)
        setattr(q, field, value)
        refused(field, x, y, edges, n_edges, q)
    q = ccdgpu.train_params(n_trees=(2 ** 31 - 1) // 2047 + 1, max_depth=10)
    refused('n_trees', x, y, edges, n_edges, q)
    q.n_trees -= 1
    assert _check(x, y, edges, n_edges, q)[0] == 0
    # 63 edges is the most
    many = np.arange(63, dtype=np.float64)
    assert _check(x[:, :1].copy(), y, many, np.array([63], np.int32), p)[0] == 0
    with pytest.raises(ValueError, match='labels'):
        ccdgpu.train_check(x, y, [[1.0, 2.0], [], [5.0]], n_classes=2)
    ccdgpu.train_check(x, y, [[1.0, 2.0], [], [5.0]], n_trees=2, features_per_node='all')


def test_reference_grows_the_perfect_tree():
    """600 rows of 33 features on 12 integer levels, label x[:, 7] // 3, depth 3, all features, no
    bootstrap: one 7-node tree that splits only on feature 7 and classifies its training rows exactly."""
    x, y, edges = tu.perfect_case()
    f = tu.train(x, y, edges, n_trees=1, max_depth=3, features_per_node=33, bootstrap=0)
    assert f.feature.shape[0] == 7 and f.root.tolist() == [0]
    assert sorted(f.feature.tolist()) == [-1, -1, -1, -1, 7, 7, 7]
    assert sorted(f.threshold[f.feature >= 0].tolist()) == [2.5, 5.5, 8.5]
    raw = forest_util.walk_raw(f, x)
    assert np.array_equal(np.argmax(raw, axis=1), y) and np.all(raw.max(axis=1) == 1.0)
    assert np.all(f.value.sum(axis=1) == 1.0)
    randomforest.Forest.from_arrays(*f.args())  # ccdgpu_forest_check passes on the reference's numbering


def test_reference_properties():
    """The restatement against itself: the trees of a forest do not depend on how many are grown; the
    parameters bind (depth, node size, gain); an empty bag is named."""
    rng = np.random.default_rng(11)
    x = rng.normal(size=(300, 5))
    y = ((x[:, 0] > 0) * 2 + (x[:, 1] + 0.3 * x[:, 2] > 0)).astype(np.int32)
    edges = randomforest.find_splits(x, 16)
    a = tu.train(x, y, edges, n_trees=5, max_depth=4, seed=9)
    b = tu.train(x, y, edges, n_trees=3, max_depth=4, seed=9)
    assert tu.equal(tu.first_trees(a, 3), b) == []
    assert tu.equal(a, tu.train(x, y, edges, n_trees=5, max_depth=4, seed=10)) != []
    randomforest.Forest.from_arrays(*a.args())
    assert randomforest.Forest(*a.args()).max_depth == 4
    one = tu.train(x, y, edges, n_trees=2, max_depth=0)
    assert one.feature.tolist() == [-1, -1] and np.allclose(one.value.sum(axis=1), 1.0)
    big = tu.train(x, y, edges, n_trees=1, max_depth=10, features_per_node=5, bootstrap=0, min_instances_per_node=40)
    leaves = big.feature < 0
    # counts of the leaves: every node holds at least 40 rows
    raw = forest_util.walk_raw(big, x)
    _, per_leaf = np.unique(raw, axis=0, return_counts=True)
    assert leaves.sum() >= 2 and per_leaf.min() >= 40
    none = tu.train(x, y, edges, n_trees=1, max_depth=10, features_per_node=5, bootstrap=0, min_info_gain=1e9)
    assert none.feature.tolist() == [-1]
    t = next(t for t in range(64) if tu.weights(0, t, 1, 1)[0] == 0)
    with pytest.raises(tu.EmptyBag) as err:
        tu.train(x[:1], y[:1], edges, n_classes=4, n_trees=t + 1)
    assert err.value.args[0] == t


def test_native_train_checks_under_sanitizers(tmp_path):
    """tests/native/train_checks.cpp: ccdgpu_train_check (csrc/ccdgpu_checks.cpp, no HIP in it) in a
    stand-alone program built with -fsanitize=address,undefined -- every argument in a heap block of
    exactly its size."""
    csrc = os.path.join(ROOT, 'lcmap-firebird_amd', 'csrc')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    probe = subprocess.run(['gcc', '-fsanitize=address,undefined', '-x', 'c', '-o', str(tmp_path / 'probe'), '-'],
                           input='int main(void){return 0;}', capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip('the compiler cannot link -fsanitize=address,undefined')
    exe = str(tmp_path / 'train_checks')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17'] + san + ['-I', os.path.join(ROOT, 'include'), '-o', exe,
                                                               os.path.join(HERE, 'native', 'train_checks.cpp'),
                                                               os.path.join(csrc, 'ccdgpu_checks.cpp')], check=True)
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith('ok'), out.stdout
