"""The random forest's bin edges, host side: the position form of the rule (include/ccdgpu.h, restated
in tests/splits_util.py -- what the device computes) against ccdc.randomforest.find_splits on every
column kind the device tests use, every refusal of ccdgpu_splits_check through ctypes (no device
needed), and the stand-alone sanitizer program of the check.  The device comparisons are in
tests/test_gpu_randomforest_splits.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ccdgpu
import splits_util as su
from ccdgpu import abi
from ccdc import randomforest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('max_bins', [2, 3, 4, 32, 64])
@pytest.mark.parametrize('n', [130, 1000])
def test_position_form_equals_the_host_rule_on_every_column_kind(n, max_bins):
    cols = su.kinds(n, max_bins, seed=n + max_bins)
    x = np.stack(list(cols.values()), axis=1)
    ref, got = su.host(x, max_bins), su.find_splits(x, max_bins)
    for name, a, b in zip(cols, ref, got):
        assert a.dtype == b.dtype and np.array_equal(a, b), (name, a, b)
    assert su.same(ref, got)
    by = dict(zip(cols, ref))
    assert by['constant'].shape == (0,)
    assert by['distinct_-1'].shape[0] == max_bins - 2 and by['distinct_+0'].shape[0] == max_bins - 1
    assert by['distinct_+1'].shape[0] <= max_bins - 1
    assert all(e.shape[0] <= max_bins - 1 and np.all(np.diff(e) > 0) for e in ref)
    if max_bins >= 32:
        assert np.isinf(by['huge_both_sides'][0]) and np.isinf(by['huge_both_sides'][-1])  # -inf and +inf edges
        assert by['neighbouring_doubles'].shape[0] < 5  # five boundaries, a repeated midpoint dropped
        assert by['both_signs_and_zeros'].tolist() == [-2.5, -1.5, -0.5, 0.5, 1.5, 2.5]  # -0.0 and +0.0 are one value


@pytest.mark.parametrize('n', [0, 1, 2, 3])
def test_position_form_on_the_smallest_columns(n):
    x = np.array([[2.0, -0.0], [1.0, 0.0], [2.0, 5e-324]])[:n]
    for max_bins in (2, 64):
        assert su.same(su.host(x, max_bins), su.find_splits(x, max_bins))


def test_position_form_on_the_hand_case():
    x = np.asarray(su.HAND).reshape(-1, 1)
    (e,) = su.find_splits(x, 4)
    assert e.tolist() == [0.5, 1.5, 2.5]
    assert su.same(su.host(x, 4), [e])


def test_position_form_on_random_cases():
    """Small random columns over few values with every max_bins: ties at every target."""
    rng = np.random.default_rng(5)
    for _ in range(300):
        n, k, mb = int(rng.integers(1, 80)), int(rng.integers(1, 40)), int(rng.integers(2, 65))
        x = rng.integers(0, k, size=(n, 2)).astype(np.float64) * rng.choice([1.0, 5e-324, 4e306])
        assert su.same(su.host(x, mb), su.find_splits(x, mb)), (n, k, mb)


def test_header_states_the_limits_the_binding_uses():
    text = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    assert 'int ccdgpu_splits_check(const double *x, int64_t n_rows, int32_t n_features, int32_t max_bins);' in text
    assert re.search(r'max_bins 2 \.\. CCDGPU_TRAIN_MAX_EDGES \+ 1', text)
    assert abi.TRAIN_MAX_EDGES + 1 == 64
    assert list(abi.SIGNATURES).index('ccdgpu_forest_find_splits') == list(abi.SIGNATURES).index('ccdgpu_splits_check') + 1


def _check(x, n_rows=None, nf=None, max_bins=32):
    rc = ccdgpu.lib().ccdgpu_splits_check(None if x is None else x.ctypes.data, x.shape[0] if n_rows is None else n_rows,
                                          x.shape[1] if nf is None else nf, max_bins)
    return rc, ccdgpu.last_error()


def test_splits_check_accepts_and_refuses():
    x = np.arange(12, dtype=np.float64).reshape(4, 3)
    assert _check(x)[0] == 0
    assert _check(x, max_bins=2)[0] == 0 and _check(x, max_bins=64)[0] == 0
    assert _check(x, n_rows=0)[0] == 0
    rc = ccdgpu.lib().ccdgpu_splits_check(None, 0, 3, 32)  # no rows: x is not read
    assert rc == 0

    def refused(needle, *args, **kw):
        rc, msg = _check(*args, **kw)
        assert rc == abi.E_INVAL and msg.startswith('splits: ') and needle in msg, (needle, rc, msg)

    rc = ccdgpu.lib().ccdgpu_splits_check(None, 4, 3, 32)
    assert rc == abi.E_INVAL and 'x is NULL' in ccdgpu.last_error()
    refused('n_rows must be in [0, 2^27], got -1', x, n_rows=-1)
    refused('n_rows must be in [0, 2^27], got %d' % ((1 << 27) + 1), x, n_rows=(1 << 27) + 1)
    refused('n_features must be in [1, 64], got 0', x, nf=0)
    refused('n_features must be in [1, 64], got 65', x, nf=65)
    refused('max_bins must be in [2, 64], got 1', x, max_bins=1)
    refused('max_bins must be in [2, 64], got 65', x, max_bins=65)
    for bad in (np.nan, np.inf, -np.inf):
        x2 = x.copy()
        x2[3, 1] = bad
        refused('x[3][1] is not finite', x2)
    x2 = x.copy()
    x2[0, 0] = np.nan
    x2[3, 2] = np.nan
    refused('x[0][0] is not finite', x2)  # the first one in row-major order
    with pytest.raises(ValueError, match=r'splits: x\[3\]\[1\] is not finite'):
        x2 = x.copy()
        x2[3, 1] = np.nan
        ccdgpu.splits_check(x2)
    with pytest.raises(ValueError, match='max_bins'):
        ccdgpu.splits_check(x, max_bins=65)
    with pytest.raises(ValueError, match='n_rows'):
        ccdgpu.splits_check(np.zeros(3))
    ccdgpu.splits_check(x, 4)
    ccdgpu.splits_check(np.zeros((0, 5)))


def test_train_refuses_an_unknown_splits_mode():
    with pytest.raises(ValueError, match="splits must be 'host' or 'device'"):
        randomforest.train(None, splits='spark')


def test_native_splits_checks_under_sanitizers(tmp_path):
    """tests/native/splits_checks.cpp: ccdgpu_splits_check (csrc/ccdgpu_checks.cpp, no HIP in it) in a
    stand-alone program built with -fsanitize=address,undefined -- x in a heap block of exactly its
    size."""
    csrc = os.path.join(ROOT, 'lcmap-firebird_amd', 'csrc')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    probe = subprocess.run(['gcc', '-fsanitize=address,undefined', '-x', 'c', '-o', str(tmp_path / 'probe'), '-'],
                           input='int main(void){return 0;}', capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip('the compiler cannot link -fsanitize=address,undefined')
    exe = str(tmp_path / 'splits_checks')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17'] + san + ['-I', os.path.join(ROOT, 'include'), '-o', exe,
                                                               os.path.join(HERE, 'native', 'splits_checks.cpp'),
                                                               os.path.join(csrc, 'ccdgpu_checks.cpp')], check=True)
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith('ok'), out.stdout
