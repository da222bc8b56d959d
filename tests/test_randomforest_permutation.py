"""Out-of-bag permutation importances, host side: every refusal of ccdgpu_permutation_check through ctypes
(no device needed) and in a stand-alone program under sanitizers, the rule's donor map, the host
arithmetic of ccdc.randomforest.permutation_summary by hand, ``Forest.save`` / ``load`` with a trained
forest's seed, bootstrap and counts, and ``permutation_importances``' own refusals.  The device
comparisons are in tests/test_gpu_randomforest_permutation.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ccdgpu
import permutation_util as pu
import train_util as tu
from ccdgpu import abi
from ccdc import randomforest
from ccdc.randomforest import Forest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def test_abi_mirrors_the_header():
    text = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    body = text[text.index('typedef struct ccdgpu_permutation_params'):text.index('} ccdgpu_permutation_params;')]
    assert re.findall(r'\b(\w+);', re.sub(r'/\*.*?\*/', '', body)) == [n for n, _ in abi.PermutationParams._fields_]
    assert ctypes.sizeof(abi.PermutationParams) == 16
    c = int(re.search(r'#define CCDGPU_PERM_HASH_C (\d+)ull', text).group(1))
    assert c == abi.PERM_HASH_C == pu.HASH_C == 2 ** 32


def _check(x, y, n_rows, nf, nc, p, outs):
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = ccdgpu.lib().ccdgpu_permutation_check(ptr(x), ptr(y), n_rows, nf, nc, None if p is None else ctypes.byref(p),
                                               *[ptr(o) for o in outs])
    return rc, ccdgpu.last_error()


def _params(seed=0, perm_seed=0):
    p = abi.PermutationParams()
    p.seed, p.perm_seed = seed, perm_seed
    return p


def test_permutation_check_accepts_and_refuses():
    x, y = np.zeros((4, 2)), np.array([0, 1, 2, 1], dtype=np.int32)
    o = [np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(6, np.int64), np.zeros(6, np.int64)]
    top = abi.TRAIN_MAX_ROWS
    assert _check(x, y, 4, 2, 3, _params(), o)[0] == 0
    assert _check(x, y, 4, 2, 3, _params(2 ** 64 - 1, 2 ** 64 - 1), o)[0] == 0
    assert _check(None, None, 0, 2, 3, _params(), o)[0] == 0          # no rows: nothing to read
    x[1, 1] = np.nan
    assert _check(x, y, 4, 2, 3, _params(), o)[0] == 0                # x is not scanned: the walk defines NaN

    def refused(needle, *args):
        rc, msg = _check(*args)
        assert rc == abi.E_INVAL and msg.startswith('permutation: ') and needle in msg, (needle, rc, msg)

    refused('params is NULL', x, y, 4, 2, 3, None, o)
    refused('x is NULL', None, y, 4, 2, 3, _params(), o)
    refused('labels is NULL', x, None, 4, 2, 3, _params(), o)
    for i, name in enumerate(('oob_rows', 'correct', 'lost', 'gained')):
        refused(name + ' is NULL', x, y, 4, 2, 3, _params(), o[:i] + [None] + o[i + 1:])
        refused(name + ' is NULL', None, None, 0, 2, 3, _params(), o[:i] + [None] + o[i + 1:])
    refused('n_rows', x, y, -1, 2, 3, _params(), o)
    refused('n_rows', x, y, top + 1, 2, 3, _params(), o)
    refused('n_features', x, y, 4, 0, 3, _params(), o)
    refused('n_features', x, y, 4, 65, 3, _params(), o)
    refused('n_classes', x, y, 4, 2, 0, _params(), o)
    refused('n_classes', x, y, 4, 2, 33, _params(), o)
    refused('labels[2] = 2', x, y, 4, 2, 2, _params(), o)             # a label equal to n_classes, with its index
    y[3] = -1
    refused('labels[3] = -1', x, y, 4, 2, 3, _params(), o)


def test_native_permutation_checks_under_sanitizers(tmp_path):
    """tests/native/permutation_checks.cpp: ccdgpu_permutation_check (csrc/ccdgpu_checks.cpp, no HIP in it)
    and the kernel's donor arithmetic (csrc/ccd_train.h) in a stand-alone program built with
    -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, 'lcmap-firebird_amd', 'csrc')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    probe = subprocess.run(['gcc', '-fsanitize=address,undefined', '-x', 'c', '-o', str(tmp_path / 'probe'), '-'],
                           input='int main(void){return 0;}', capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip('the compiler cannot link -fsanitize=address,undefined')
    exe = str(tmp_path / 'permutation_checks')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17'] + san + ['-I', os.path.join(ROOT, 'include'), '-o', exe,
                                                               os.path.join(HERE, 'native', 'permutation_checks.cpp'),
                                                               os.path.join(csrc, 'ccdgpu_checks.cpp')], check=True)
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith('ok'), out.stdout


@pytest.mark.parametrize('n', [1, 2, 3, 64, 600, 1000])
def test_the_donor_map_is_a_bijection_and_the_stated_formula(n):
    for perm_seed, t, f in ((0, 0, 0), (11, 3, 7), (2 ** 64 - 1, 499, 63)):
        d = pu.donors(perm_seed, t, f, n)
        assert d.dtype == np.uint64 and np.array_equal(np.sort(d), np.arange(n, dtype=np.uint64))
        # the formula of include/ccdgpu.h, in Python integers
        k = int(tu.H(perm_seed, t, f, 2 ** 32))
        b, a = (k >> 32) % n, (k & 0xffffffff) % n
        while math.gcd(a, n) != 1:
            a = a + 1 if a + 1 < n else 0
        assert (a, b) == pu.pair(perm_seed, t, f, n)
        assert d.tolist() == [(a * r + b) % n for r in range(n)]
        if n == 1:
            assert (a, b) == (0, 0) and d.tolist() == [0]
    if n >= 600:  # different columns and trees are shuffled differently
        assert not np.array_equal(pu.donors(5, 0, 0, n), pu.donors(5, 0, 1, n))
        assert not np.array_equal(pu.donors(5, 0, 0, n), pu.donors(5, 1, 0, n))
        assert not np.array_equal(pu.donors(5, 0, 0, n), pu.donors(6, 0, 0, n))


def test_summary_by_hand():
    """Three trees, two features, three classes.  Tree 1 has no out-of-bag row and is left out; no tree
    saw class 2.  Tree 0: N = 10 (6 + 4); feature 0 loses 3 + 1 and gains 1 + 0: d = 3/10; feature 1: 0.
    Tree 2: N = 4 (4 + 0); feature 0 loses 1: d = 1/4; feature 1 gains 2: d = -2/4."""
    oob_rows = np.array([[6, 4, 0], [0, 0, 0], [4, 0, 0]])
    correct = np.array([[5, 2, 0], [0, 0, 0], [2, 0, 0]])
    lost = np.array([[[3, 1, 0], [0, 0, 0]], [[0, 0, 0], [0, 0, 0]], [[1, 0, 0], [0, 0, 0]]])
    gained = np.array([[[1, 0, 0], [0, 0, 0]], [[0, 0, 0], [0, 0, 0]], [[0, 0, 0], [2, 0, 0]]])
    s = randomforest.permutation_summary(oob_rows, correct, lost, gained)
    assert s.trees_used == 2
    assert s.importances.dtype == np.float64
    assert s.importances.tolist() == [(3 / 10 + 1 / 4) / 2, (0.0 + -2 / 4) / 2]
    m0, m1 = s.importances.tolist()
    assert s.importances_std.tolist() == [math.sqrt(((3 / 10 - m0) ** 2 + (1 / 4 - m0) ** 2) / 1),
                                          math.sqrt(((0.0 - m1) ** 2 + (-2 / 4 - m1) ** 2) / 1)]
    # class 0: trees 0 and 2; class 1: tree 0 only; class 2: no tree
    assert s.class_importances.shape == (3, 2)
    assert s.class_importances[0].tolist() == [((3 - 1) / 6 + 1 / 4) / 2, (0.0 + -2 / 4) / 2]
    assert s.class_importances[1].tolist() == [1 / 4, 0.0]
    assert np.all(np.isnan(s.class_importances[2]))
    for name, given in (('oob_rows', oob_rows), ('correct', correct), ('lost', lost), ('gained', gained)):
        assert getattr(s, name).dtype == np.int64 and np.array_equal(getattr(s, name), given)
    ref = pu.importances(oob_rows, lost, gained)
    assert np.array_equal(s.importances, ref[0]) and np.array_equal(s.importances_std, ref[1])
    assert np.array_equal(s.class_importances, ref[2], equal_nan=True) and s.trees_used == ref[3]


def test_summary_below_two_trees_and_without_any():
    one = randomforest.permutation_summary([[0, 0], [2, 2]], [[0, 0], [1, 2]], [[[0, 0]], [[1, 0]]], [[[0, 0]], [[0, 0]]])
    assert one.trees_used == 1 and one.importances.tolist() == [0.25] and np.isnan(one.importances_std[0])
    assert one.class_importances.tolist() == [[0.5], [0.0]]
    none = randomforest.permutation_summary(np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 3, 2)), np.zeros((2, 3, 2)))
    assert none.trees_used == 0 and np.all(np.isnan(none.importances)) and np.all(np.isnan(none.importances_std))
    assert np.all(np.isnan(none.class_importances)) and none.class_importances.shape == (2, 3)
    with pytest.raises(ValueError):
        randomforest.permutation_summary(np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 3, 3)), np.zeros((2, 3, 3)))
    with pytest.raises(ValueError):
        randomforest.permutation_summary(np.zeros((2, 2)), np.zeros((2, 3)), np.zeros((2, 3, 2)), np.zeros((2, 3, 2)))


def _stump():
    return Forest.from_arrays([0], [1, -1, -1], [0.5, 0.0, 0.0], [1, -1, -1], [2, -1, -1], [[0.5, 0.5], [1, 0], [0, 1]], 3)


def test_save_and_load_keep_what_a_trained_forest_carries(tmp_path):
    plain = _stump()
    plain.save(str(tmp_path / 'plain'))
    with np.load(str(tmp_path / 'plain.npz')) as z:
        assert sorted(z.files) == sorted(['n_features', 'root', 'feature', 'threshold', 'left', 'right', 'value'])
    back = Forest.load(str(tmp_path / 'plain.npz'))
    assert tu.equal(back, plain) == [] and back.seed is None and back.bootstrap is None and back.counts is None
    trained = _stump()
    trained.seed, trained.bootstrap = 2 ** 64 - 1, True
    trained.counts = np.array([[4, 4], [4, 0], [0, 4]], dtype=np.int64)
    trained.save(str(tmp_path / 'trained'))
    back = Forest.load(str(tmp_path / 'trained.npz'))
    assert tu.equal(back, trained) == [] and back.n_features == 3
    assert back.seed == 2 ** 64 - 1 and type(back.seed) is int and back.bootstrap is True
    assert back.counts.dtype == np.int64 and np.array_equal(back.counts, trained.counts)
    assert randomforest.feature_importances(back).tolist() == [0.0, 1.0, 0.0]
    # each of the three on its own
    partly = _stump()
    partly.seed, partly.bootstrap = 0, False
    partly.save(str(tmp_path / 'partly'))
    back = Forest.load(str(tmp_path / 'partly.npz'))
    assert back.seed == 0 and back.bootstrap is False and back.counts is None


def test_permutation_importances_refuses_a_forest_without_bags_or_seed():
    """Before anything reaches a device."""
    f = _stump()
    x, y = np.zeros((2, 3)), [0, 1]
    with pytest.raises(ValueError, match='seed'):
        randomforest.permutation_importances(f, x, y)
    f.seed, f.bootstrap = 5, False
    with pytest.raises(ValueError, match='bootstrap'):
        randomforest.permutation_importances(f, x, y)
    with pytest.raises(ValueError, match='bootstrap'):
        randomforest.permutation_importances(f, x, y, seed=1)
    with pytest.raises(ValueError, match='bootstrap'):
        randomforest.train(None, bootstrap=False, permutation=True)
