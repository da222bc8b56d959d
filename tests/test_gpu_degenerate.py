"""GPU parity on zero-variogram, flat and exact-fit pixels (tests/degenerate_util.py): inputs that
reach the detection kernel's NaN / inf branches -- a zero variogram in the batched lookforward's
bounds, max(rmse, vario) == 0 in stable(), NaN comparison rmse, w_max == 0 in the descent's
stopping test -- which no noisy input does.

The *defined* pixels are held to the project's parity bar against the C oracle (integers and
masks exact, floats within parity_util.RTOL / ATOL), under three parameter sets and two pixel
orders, each pixel alone in its launch, and through both transport encodings.  The
*rounding-decided* pixels (A, E, F, G) have no parity bar (Tmask's |pred - obs| > 0 on a constant
band is the rounding of a least-squares solve); the kernel must end and return well-formed
results on them."""
import functools

import numpy as np
import pytest

import ccdgpu
import degenerate_util as du
import oracle_ctypes
import pack_util
import parity_util

pytestmark = pytest.mark.gpu

ORACLE_THREADS = 16
PARAMS = [None, {'ARGSORT': 'stable'}, {'RMSE_DOF': True}]
PARAM_IDS = ['default', 'argsort_stable', 'rmse_dof']


@pytest.fixture(scope='module')
def ctx():
    c = ccdgpu.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def defined(cadence):
    return du.defined(cadence)


@functools.lru_cache(maxsize=None)
def oracle(cadence, which):
    """the C oracle's result on the defined pixels in recipe order, computed once per parameter set"""
    d, s, q = defined(cadence)
    rc, ref = oracle_ctypes.detect_batch(d, s, q, params=PARAMS[which], threads=ORACLE_THREADS)
    assert rc == 0
    return ref


def assert_parity(got, ref):
    problems, max_rel = parity_util.compare(got, ref)
    assert not problems, problems[:10]
    assert max_rel < parity_util.RTOL


def segments_of(u, px):
    x = u.segments[u.seg_offsets[px]:u.seg_offsets[px + 1]].copy()
    x['pixel'] = 0
    return x


@pytest.mark.parametrize('reverse', [False, True], ids=['recipe_order', 'reversed'])
@pytest.mark.parametrize('which', range(len(PARAMS)), ids=PARAM_IDS)
@pytest.mark.parametrize('cadence', ['16d', '4d'])
def test_defined_pixels_match_the_oracle(ctx, cadence, which, reverse):
    d, s, q = defined(cadence)
    ref = oracle(cadence, which)
    if reverse:  # other neighbours in the launch: the oracle runs on the reversed batch itself
        s, q = np.ascontiguousarray(s[:, ::-1]), np.ascontiguousarray(q[::-1])
        rc, ref_r = oracle_ctypes.detect_batch(d, s, q, params=PARAMS[which], threads=ORACLE_THREADS)
        assert rc == 0
        n = q.shape[0]
        for px in range(n):  # (and gives each pixel what it gave it in recipe order)
            assert segments_of(ref_r, px).tobytes() == segments_of(ref, n - 1 - px).tobytes()
        ref = ref_r
    got = ctx.detect_batch(d, s, q, params=PARAMS[which])
    assert_parity(got, ref)
    assert np.array_equal(got.probs, ref.probs) or np.allclose(got.probs, ref.probs, rtol=parity_util.RTOL, atol=0.0)
    for f in parity_util.FLOAT_FIELDS:
        assert np.isfinite(got.segments[f]).all(), f


@pytest.mark.parametrize('cadence', ['16d', '4d'])
def test_each_defined_pixel_alone_equals_its_result_in_the_batch(ctx, cadence):
    d, s, q = defined(cadence)
    full = ctx.detect_batch(d, s, q)
    for px in range(q.shape[0]):
        one = ctx.detect_batch(d, s[:, px:px + 1], q[px:px + 1])
        name = du.DEFINED[cadence][px].name
        assert one.segments.tobytes() == segments_of(full, px).tobytes(), name
        assert np.array_equal(one.mask[0], full.mask[px]), name
        assert one.procedure[0] == full.procedure[px], name


def _staged(c, slot, batch):
    c.stage_slot_chips(slot, batch)
    c.run_slot(slot)
    s, q = c.staged_inputs()
    return s, q, [c.fetch(k) for k in range(batch.n_chips)]


@pytest.mark.parametrize('pack', [False, True], ids=['plain', 'packed'])
def test_encoded_batch_stages_the_raw_inputs_and_detects_the_same(pack):
    """Both date sets as the two chips of one batch through EncodedBatch.encode, plain (mode 1)
    and bit-packed (mode 2: flat and two-level bands are its widths 0 and 1): the staged inputs
    equal the raw upload's, the segments are identical, and they are detect_batch's."""
    cs = [defined('16d'), defined('4d')]
    raw = ccdgpu.ChipBatch.from_chips(cs, pinned=True)
    enc = ccdgpu.EncodedBatch.encode(cs, threads=4, pack=pack)
    assert enc.chip_modes() == [2 if pack else 1] * 2
    if pack:
        assert {0, 1} <= set(pack_util.widths(enc.buf[:enc.nbytes_encoded]).tolist())
    c = ccdgpu.Context(0)
    try:
        s0, q0, r0 = _staged(c, 0, raw)
        s1, q1, r1 = _staged(c, 1, enc)
        direct = [c.detect_batch(*chip) for chip in cs]
    finally:
        c.close()
    np.testing.assert_array_equal(q0, np.asarray(raw.qa))
    np.testing.assert_array_equal(s0, np.asarray(raw.spectra))
    np.testing.assert_array_equal(q1, q0)
    np.testing.assert_array_equal(s1, s0)
    for a, b, u in zip(r0, r1, direct):
        assert a.segments.tobytes() == b.segments.tobytes() == u.segments.tobytes()
        assert np.array_equal(a.seg_offsets, b.seg_offsets) and np.array_equal(a.seg_offsets, u.seg_offsets)
        assert np.array_equal(a.procedure, b.procedure) and np.array_equal(a.procedure, u.procedure)
        assert np.array_equal(a.mask, b.mask) and np.array_equal(a.mask, u.mask)


@pytest.mark.parametrize('cadence', ['16d', '4d'])
def test_rounding_decided_pixels_end_with_well_formed_results(ctx, cadence):
    """A, E, F, G: no parity bar, but the launch returns (detect_batch raises on any return code
    but 0), the procedure is the oracle's (it depends on QA alone), the mask stays inside the
    standard filter's keep set, every segment lies on the pixel's dates with no more observations
    than the mask holds, every float is finite, and a pixel alone gives the bytes it gives in the
    batch.

    Why the kernel's loops end on these inputs, whatever NaN or inf their operands hold
    (lcmap-firebird_amd/csrc/ccd_kernels.hip):
    * Tmask IRLS (tmask, tmask_reg, tmask_pair): ``while (!converged && iteration < 5)``, and
      every pass adds 1 to ``iteration``; a NaN makes ``coef - coef0 > 1e-8`` false, which only
      ends the loop sooner.  A constant band has y-std 0 and mad 0, so scale = 0 and u = r / 0 is
      NaN or inf: ``fabs(u) < 4.685`` is false, every weight 0, the normal matrix 0, chol5's
      ``!(d > 0)`` refuses it (a NaN pivot too) and tm_solve returns zero coefficients.  The
      medians are a fixed bitonic network or kth_nonneg, a bisection over the 63 value bits.
    * the descent (cd_sweep, spec_fits): ``for (it = 0; it < max_iter; ++it)`` with max_iter =
      LASSO_MAX_ITER; the stopping tests only leave it sooner.  A constant band has y'y = 0 and
      w_max = 0: the duality gap 0 is not below tol * y'y = 0, so it runs all max_iter sweeps, as
      the reference's does.
    * initialize's window walk: every ``continue`` first moves the window's end one observation
      on (a short span, all rows flagged, too few rows kept, or an unstable fit -- the NaN of
      0 / max(rmse, vario) = 0 / 0 in stable() makes ``sqrt(sum) < threshold`` false), and
      ``b + MEOW_SIZE < m`` bounds it by the period's length m, which only shrinks.
    * lookback steps its window start down to the previous break; ``!(mag > threshold)`` and
      ``mag0 > outlier`` are both plain "no" for a NaN magnitude.  Every lookforward step adds
      one observation to the window, drops one from the period or ends the segment, bounded by
      m the same way."""
    d, s, q = du.rounding_decided(cadence)
    rc, ref = oracle_ctypes.detect_batch(d, s, q, threads=4)
    assert rc == 0
    got = ctx.detect_batch(d, s, q)
    assert np.array_equal(got.procedure, ref.procedure)
    assert np.array_equal(got.sorted_dates, np.sort(d))
    for px, r in enumerate(du.ROUNDING):
        keep = du.standard_filtered(d, s[:, px], q[px])[2]
        assert not (got.mask[px] & ~keep).any(), r.name
        sg = segments_of(got, px)
        assert (sg['start_day'] <= sg['end_day']).all(), r.name
        assert np.isin(sg['start_day'], d).all() and np.isin(sg['end_day'], d).all(), r.name
        assert (sg['observation_count'] <= got.mask[px].sum()).all() and (sg['observation_count'] > 0).all(), r.name
        for f in parity_util.FLOAT_FIELDS:
            assert np.isfinite(sg[f]).all(), (r.name, f)
        one = ctx.detect_batch(d, s[:, px:px + 1], q[px:px + 1])
        assert one.segments.tobytes() == sg.tobytes(), r.name
        assert np.array_equal(one.mask[0], got.mask[px]), r.name
    assert np.isfinite(got.probs).all()


_GUARD_SCRIPT = r'''
import hashlib, sys
sys.path[:0] = sys.argv[1:]
import ccdgpu, degenerate_util as du
c = ccdgpu.Context(0)
h = hashlib.sha256()
for cadence in ('16d', '4d'):
    u = c.detect_batch(*du.rounding_decided(cadence))
    for a in (u.seg_offsets, u.segments, u.mask, u.procedure):
        h.update(a.tobytes())
c.close()
print(h.hexdigest())
'''


def test_rounding_decided_pixels_trip_no_guard_in_the_checking_build(ctx):
    """In bounds: the checking build (lib/libccdgpu_guard.so raises CCDGPU_EHIP naming the line of
    any tripped index guard or partial-EXEC cross-lane operation; the defined pixels run through
    it as goldens, test_gpu_batches.py) trips none on the rounding-decided pixels, in a child
    process (the library is chosen at load), and gives the product build's bytes."""
    import hashlib
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    guard = os.path.join(root, 'lcmap-firebird_amd', 'lib', 'libccdgpu_guard.so')
    assert os.path.exists(guard), 'build lib/libccdgpu_guard.so (make -C lcmap-firebird_amd)'
    paths = [os.path.join(root, 'lcmap-firebird_amd'), os.path.join(root, 'tests')]
    r = subprocess.run([sys.executable, '-c', _GUARD_SCRIPT] + paths, env=dict(os.environ, CCDGPU_LIBRARY=guard),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    h = hashlib.sha256()
    for cadence in ('16d', '4d'):
        u = ctx.detect_batch(*du.rounding_decided(cadence))
        for a in (u.seg_offsets, u.segments, u.mask, u.procedure):
            h.update(a.tobytes())
    assert r.stdout.strip().splitlines()[-1] == h.hexdigest()
