"""CPU tests of the degenerate detection inputs (tests/degenerate_util.py) and of the parity
comparator's handling of non-finite values.  The inputs must be what their recipes claim -- a
zero adjusted variogram in the named bands, all three procedures, every curve_qa, a break found
next to a zero-variogram detection band and a break suppressed by a flat one -- or the GPU tests
built on them (tests/test_gpu_degenerate.py, test_gpu.py::test_golden[degenerate_*]) check nothing
new.  Every expectation here is computed from the numpy restatement (oracle/ccd_ref.py) alone."""
import copy
import warnings

import numpy as np
import pytest

import ccd_ref
import degenerate_util as du
import golden_util
import parity_util
from ccdgpu import abi

GOLDENS = (('degenerate_16d', '16d'), ('degenerate_4d', '4d'), ('degenerate_16d_allbands', '16d'))


standard_filtered = du.standard_filtered


def variogram(d, s_px, q_px):
    dates, obs, _ = standard_filtered(d, s_px, q_px)
    return ccd_ref.adjusted_variogram(dates, obs)


def segments_of(u, px):
    return u.segments[u.seg_offsets[px]:u.seg_offsets[px + 1]]


@pytest.mark.parametrize('cadence', ['16d', '4d'])
def test_defined_pixels_have_the_variograms_their_recipes_name(cadence):
    d, s, q = du.defined(cadence)
    recipes = du.DEFINED[cadence]
    assert q.shape == (len(recipes), len(du.DATES[cadence])) and d.shape[0] in (230, 520)
    for px, r in enumerate(recipes):
        v = variogram(d, s[:, px], q[px])
        if r.zero is not None:
            assert set(r.zero) | set(r.noisy) == set(du.ALL)
            for b in r.zero:
                assert v[b] == 0.0, (r.name, b, v)
            for b in r.noisy:
                assert v[b] > 0.0, (r.name, b, v)
        if r.name == 'I':
            # one-count noise: each band's variogram is 0 or 1 count (thermal: 10, Celsius x 100);
            # above 0 in the Tmask bands (at 0 there the pixel would be rounding-decided), and at
            # the 16-day dates 0 in a detection band
            assert set(v[:6]) <= {0.0, 1.0} and v[6] in (0.0, 10.0), v
            assert all(v[b] > 0.0 for b in du.TMASK_BANDS), v
            if cadence == '16d':
                assert any(v[b] == 0.0 for b in (2, 3, 5)), v


def test_filter_boundary_values_are_dropped_and_kept_as_recipe_q_says():
    d, s, q = du.defined('16d')
    n = d.shape[0]
    _, _, mask = standard_filtered(d, s[:, du.index(du.DEFINED_16D, 'Q')], q[du.index(du.DEFINED_16D, 'Q')])
    expect = np.ones(n, dtype=bool)
    plan = du.q_plan(n)
    assert {(v, k) for _, _, v, k in plan} == set(du.Q_VALUES) | set(du.Q_THERMAL)
    for i, _, _, kept in plan:
        expect[i] = kept
    assert np.array_equal(mask, expect)
    _, _, mask = standard_filtered(d, s[:, du.index(du.DEFINED_16D, 'Q2')], q[du.index(du.DEFINED_16D, 'Q2')])
    assert np.array_equal(mask, np.arange(n) % 3 != 0)


@pytest.mark.parametrize('name,cadence', GOLDENS)
def test_goldens_hold_the_defined_inputs_and_finite_floats(name, cadence):
    (d, s, q), params, u = golden_util.load(name)
    dd, ss, qq = du.defined(cadence)
    assert np.array_equal(d, dd) and np.array_equal(s, ss) and np.array_equal(q, qq)
    for f in parity_util.FLOAT_FIELDS:
        assert np.isfinite(u.segments[f]).all(), f
    assert np.isfinite(u.probs).all()


def test_golden_coverage():
    """What the GPU tests stand on: the 16-day goldens hold all three procedures, curve_qa 8, 14,
    24, 44 and 54, a pixel with two or more segments whose detection bands include a
    zero-variogram band, a pixel whose step goes undetected (M: one segment, while M2 -- the same
    step, red two-level instead of constant -- has two) and a pixel with no model (N11)."""
    recipes = du.DEFINED_16D
    for name, cadence in GOLDENS:
        (d, s, q), params, u = golden_util.load(name)
        rec = du.DEFINED[cadence]
        det = ccd_ref.get_params(params).DETECTION_BANDS
        broken = [r.name for px, r in enumerate(rec)
                  if len(segments_of(u, px)) >= 2 and r.zero and set(r.zero) & set(det)]
        assert broken, name
        assert set(broken) <= {'M2', 'M3', 'M4', 'J'}
        assert len(segments_of(u, du.index(rec, 'M'))) == 1, name
        assert len(segments_of(u, du.index(rec, 'M2'))) == 2, name
        assert segments_of(u, du.index(rec, 'M2'))['change_probability'][0] == 1.0
    (d, s, q), params, u = golden_util.load('degenerate_16d')
    assert set(u.procedure.tolist()) == {0, 1, 2}
    assert {8, 14, 24, 44, 54} <= set(u.segments['curve_qa'].tolist())
    n11 = du.index(recipes, 'N11')
    assert u.procedure[n11] == 2 and len(segments_of(u, n11)) == 0 and u.mask[n11].sum() == 11
    # a flat detection band suppresses the break: M3 / M4 find it while their flat band (thermal,
    # blue) is no detection band, and do not with all seven
    (_, _, _), _, ua = golden_util.load('degenerate_16d_allbands')
    for nm in ('M3', 'M4'):
        assert len(segments_of(u, du.index(recipes, nm))) == 2
        assert len(segments_of(ua, du.index(recipes, nm))) == 1


def test_numpy_restatement_reproduces_degenerate_goldens():
    """a few pixels of each kind, re-run: the committed goldens are ccd_ref's results on the
    recipes' inputs"""
    (d, s, q), params, u = golden_util.load('degenerate_16d')
    for nm in ('H', 'J', 'M', 'M2', 'N11', 'S2'):
        px = du.index(du.DEFINED_16D, nm)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')  # (the reference's 0 / 0)
            r = ccd_ref.detect(d, *[s[b, px] for b in range(7)], q[px], params=params)
        assert abi.PROCEDURES.index(r['procedure']) == u.procedure[px]
        assert np.array_equal(np.array(r['processing_mask'], dtype=bool), u.mask[px])
        sg = segments_of(u, px)
        assert len(r['change_models']) == len(sg)
        for cm, g in zip(r['change_models'], sg):
            for f in parity_util.INT_FIELDS:
                assert cm[f] == g[f]
            assert [cm[b]['rmse'] for b in abi.BANDS] == g['rmse'].tolist()
            assert [cm[b]['magnitude'] for b in abi.BANDS] == g['magnitude'].tolist()


@pytest.mark.parametrize('cadence', ['16d', '4d'])
def test_rounding_decided_pixels_have_a_constant_tmask_band(cadence):
    """the stated reason for their exclusion from the parity bar: a Tmask band is constant and its
    variogram 0, so Tmask's test is |pred - obs| > 0 on the rounding of a least-squares solve (G:
    constant but for its spikes, which the robust fit weighs out)"""
    assert du.names(du.ROUNDING) == ['A', 'E', 'F', 'G']
    d, s, q = du.rounding_decided(cadence)
    for px, r in enumerate(du.ROUNDING):
        _, obs, mask = standard_filtered(d, s[:, px], q[px])
        assert mask.all()
        v = variogram(d, s[:, px], q[px])
        level = [float(np.mean(obs[b] == np.median(obs[b]))) for b in du.TMASK_BANDS]
        flat = [b for b, lv in zip(du.TMASK_BANDS, level) if v[b] == 0.0 and lv >= (0.9 if r.name == 'G' else 1.0)]
        assert flat, (r.name, v, level)


# ---- parity_util.compare and non-finite values
def _doctored(u, field, where, value):
    v = copy.copy(u)
    v.segments = u.segments.copy()
    v.segments[field][where] = value
    return v


@pytest.fixture(scope='module')
def golden():
    return golden_util.load('degenerate_16d')[2]


def test_compare_golden_with_itself(golden):
    problems, max_rel = parity_util.compare(golden, golden)
    assert problems == [] and max_rel == 0.0


@pytest.mark.parametrize('field,value', [('rmse', np.nan), ('magnitude', np.inf), ('magnitude', -np.inf),
                                         ('coef', np.nan), ('change_probability', np.nan)])
def test_compare_reports_a_non_finite_value_on_either_side(golden, field, value):
    where = (3, 2) if golden.segments[field].ndim > 1 else 3
    bad = _doctored(golden, field, where, value)
    for got, ref in ((bad, golden), (golden, bad)):
        problems, max_rel = parity_util.compare(got, ref)
        assert len(problems) == 1 and field in problems[0] and 'seg' in problems[0], problems
        assert not max_rel < parity_util.RTOL


def test_compare_matches_non_finite_values_only_with_their_own_kind(golden):
    nan = _doctored(golden, 'rmse', (3, 2), np.nan)
    pinf = _doctored(golden, 'magnitude', (5, 1), np.inf)
    ninf = _doctored(golden, 'magnitude', (5, 1), -np.inf)
    nan_there = _doctored(golden, 'magnitude', (5, 1), np.nan)
    for same in (nan, pinf, ninf):
        problems, max_rel = parity_util.compare(same, copy.copy(same))
        assert problems == [] and max_rel == 0.0
    for a, b in ((pinf, ninf), (ninf, pinf), (pinf, nan_there), (nan_there, ninf)):
        problems, max_rel = parity_util.compare(a, b)
        assert len(problems) == 1 and 'magnitude' in problems[0], problems
        assert max_rel == np.inf
    # a matched pair hides no finite difference next to it
    off = _doctored(nan, 'rmse', (3, 4), nan.segments['rmse'][3, 4] * (1 + 1e-3) + 1.0)
    problems, max_rel = parity_util.compare(off, nan)
    assert len(problems) == 1 and 'rmse' in problems[0]
    assert 1e-4 < max_rel < np.inf
