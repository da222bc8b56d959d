"""Degenerate detection inputs: pixels with a zero adjusted variogram, an exactly zero model rmse,
a two-valued Tmask band or a detection band flat through a real break (dark water, quantised
thermal data, stuck bands).  Every other input of the suite carries Gaussian noise of 30 - 150
counts per band, so none of them reaches the NaN / inf branches of the reference:
``np.min(mags) > thr`` is False when any magnitude is NaN, ``np.maximum`` propagates NaN, and the
``0 / 0`` in ``change.stable`` makes a window never stable.

One small generator per recipe, fixed seeds.  Two date sets: ``16d`` (230 observations, 16 days
apart) and ``4d`` (520 observations, 4 days apart: Tmask windows above 64 rows and an adaptive
peek of 24).  Two pixel lists per date set:

* *defined* -- the numpy restatement and the C oracle agree on them (goldens ``degenerate_*``,
  minted by tests/golden/make_golden.py); the GPU path is held to the project's parity bar.
* *rounding-decided* (A, E, F, G) -- a Tmask band is constant, its variogram 0, so Tmask keeps an
  observation iff ``|pred - obs| > 0``, where ``pred - obs`` is the rounding noise of a
  least-squares solve of an exactly representable constant.  numpy's lstsq leaves ~1e-13 on some
  rows, normal equations often exactly 0; no implementation can be asked to match that.  The GPU
  path must still end, stay in bounds and return well-formed results on them.

Every observation is clear (QA 66) unless the recipe says otherwise.  "two-level" is the base
level plus 1 with probability 0.3 (its lagged differences are 0 more often than not: variogram 0,
but a model rmse above 0); "noise" is N(0, 40), rounded."""
import numpy as np

BASE = np.array([500, 800, 700, 2800, 2000, 1200, 2950], dtype=np.int64)
ALL = (0, 1, 2, 3, 4, 5, 6)
CLEAR, SNOW, CLOUD = 66, 80, 224

DATES = {
    '16d': (724000 + 16 * np.arange(230)).astype(np.int64),
    '4d': (730000 + 4 * np.arange(520)).astype(np.int64),
}
N_LAST = (11, 12, 17, 18, 23, 24, 25, 30)  # recipes N<m>: clear observations at the series' end


# ---- building blocks (n observations -> [7][n] int64)
def constant(n):
    return np.repeat(BASE[:, None], n, axis=1)


def two_level(rng, n):
    return constant(n) + (rng.uniform(size=(7, n)) < 0.3)


def noise(rng, n):
    return constant(n) + np.round(rng.normal(0.0, 40.0, (7, n))).astype(np.int64)


def clear(n):
    return np.full(n, CLEAR, dtype=np.uint16)


def optical_step(y, at, by):
    """a step in the six optical bands (the thermal band stays: + 500 would carry it past
    THERMAL_MAX, and the standard filter would drop the series' second half)"""
    y[:6, at:] += by


# ---- the defined recipes: f(rng, dates) -> ([7][n] values, [n] qa)
def rec_B(rng, d):
    return two_level(rng, len(d)), clear(len(d))


def rec_D3(rng, d):
    n = len(d)
    y = two_level(rng, n)
    y[:, n // 3:] += 400
    y[:, 2 * n // 3:] -= 300
    return y, clear(n)


def rec_H(rng, d):
    y = noise(rng, len(d))
    y[2] = BASE[2]
    return y, clear(len(d))


def rec_I(rng, d):
    n = len(d)
    return constant(n) + np.round(rng.normal(0.0, 0.6, (7, n))).astype(np.int64), clear(n)


def rec_J(rng, d):
    n = len(d)
    y = noise(rng, n)
    y[5] = np.where(np.arange(n) < n // 2, 1200, 1600)
    return y, clear(n)


def rec_K(rng, d):
    n = len(d)
    y = noise(rng, n)
    y[[1, 4]] = two_level(rng, n)[[1, 4]]
    return y, clear(n)


def _step_with(rng, d, band, flat):
    n = len(d)
    y = noise(rng, n)
    optical_step(y, n // 2, 500)
    y[band] = (two_level(rng, n) if flat == 'two-level' else constant(n))[band]
    return y, clear(n)


def rec_M(rng, d):
    return _step_with(rng, d, 2, 'constant')


def rec_M2(rng, d):
    return _step_with(rng, d, 2, 'two-level')


def rec_M3(rng, d):
    return _step_with(rng, d, 6, 'constant')


def rec_M4(rng, d):
    return _step_with(rng, d, 0, 'constant')


def rec_C(rng, d):
    w = 2 * np.pi / 365.2425
    y = np.round(BASE[:, None] + 300.0 * np.cos(w * d[None, :].astype(np.float64))).astype(np.int64)
    return y, clear(len(d))


Q_VALUES = ((0, False), (1, True), (9999, True), (10000, False))       # (optical value, kept)
Q_THERMAL = ((1799, False), (1800, True), (3438, True))                # (thermal value, kept)


def q_plan(n):
    """[(observation, band, value, kept)] of recipe Q: every 7th observation carries one boundary
    value of the saturation / thermal-range filters, the optical ones walking over the six bands"""
    plan = []
    for k, i in enumerate(range(0, n, 7)):
        c = k % 7
        if c < 4:
            plan.append((i, (k // 7) % 6, Q_VALUES[c][0], Q_VALUES[c][1]))
        else:
            plan.append((i, 6, Q_THERMAL[c - 4][0], Q_THERMAL[c - 4][1]))
    return plan


def rec_Q(rng, d):
    n = len(d)
    y = noise(rng, n)
    for i, band, value, _ in q_plan(n):
        y[band, i] = value
    return y, clear(n)


def rec_Q2(rng, d):
    y = noise(rng, len(d))
    y[6, ::3] = 3439  # 3439 * 10 - 27315 = 7075 > THERMAL_MAX
    return y, clear(len(d))


def rec_N(m):
    def f(rng, d):
        n = len(d)
        q = np.full(n, CLOUD, dtype=np.uint16)
        q[n - m:] = CLEAR
        return two_level(rng, n), q
    f.__name__ = 'rec_N%d' % m
    return f


def _sparse_clear(n, other, every):
    q = np.full(n, other, dtype=np.uint16)
    q[::every] = CLEAR
    return q


def rec_S(rng, d):
    return two_level(rng, len(d)), _sparse_clear(len(d), SNOW, 12)


def rec_S2(rng, d):
    return constant(len(d)), _sparse_clear(len(d), SNOW, 12)


def rec_T(rng, d):
    return two_level(rng, len(d)), _sparse_clear(len(d), CLOUD, 6)


def rec_T2(rng, d):
    return constant(len(d)), _sparse_clear(len(d), CLOUD, 6)


# ---- the rounding-decided recipes
def rec_A(rng, d):
    return constant(len(d)), clear(len(d))


def rec_E(rng, d):
    y = noise(rng, len(d))
    y[[1, 4]] = BASE[[1, 4], None]
    return y, clear(len(d))


def rec_F(rng, d):
    y = constant(len(d))
    y[3] = noise(rng, len(d))[3]
    return y, clear(len(d))


def rec_G(rng, d):
    n = len(d)
    y = constant(n)
    y[:6, rng.uniform(size=n) < 0.05] += 500
    return y, clear(n)


class Recipe(object):
    """name, generator, seed, and what the recipe names: the bands whose adjusted variogram (of
    the standard-filtered observations) is 0 and those carrying noise (variogram > 0); ``None``
    where the recipe names neither (I: variograms of 0 and 1 mixed; N, S, T: procedures that use
    no variogram)"""

    def __init__(self, name, fn, seed, zero=None, noisy=None):
        self.name, self.fn, self.seed, self.zero, self.noisy = name, fn, seed, zero, noisy

    def make(self, dates, cadence):
        rng = np.random.default_rng(self.seed + (0 if cadence == '16d' else 1000))
        y, q = self.fn(rng, dates)
        assert y.min() >= -32768 and y.max() <= 32767
        return y.astype(np.int16), q


def _others(zero):
    return tuple(b for b in ALL if b not in zero)


DEFINED_16D = [
    Recipe('B', rec_B, 9001, zero=ALL, noisy=()),
    Recipe('D3', rec_D3, 9002, zero=ALL, noisy=()),
    Recipe('H', rec_H, 9003, zero=(2,), noisy=_others((2,))),
    # (a seed at which the 16-day variogram is 0 in nir and 1 in the other optical bands.  With a
    # zero variogram in a Tmask band -- seed 9354: green -- recipe I is rounding-decided: the
    # robust fit settles on the majority level exactly, and Tmask's |pred - obs| > 0 is rounding
    # there; the two restatements then disagree, as on A, E, F and G)
    Recipe('I', rec_I, 9024),
    Recipe('J', rec_J, 9005, zero=(5,), noisy=_others((5,))),
    Recipe('K', rec_K, 9006, zero=(1, 4), noisy=_others((1, 4))),
    Recipe('M', rec_M, 9007, zero=(2,), noisy=_others((2,))),
    Recipe('M2', rec_M2, 9008, zero=(2,), noisy=_others((2,))),
    Recipe('M3', rec_M3, 9009, zero=(6,), noisy=_others((6,))),
    Recipe('M4', rec_M4, 9010, zero=(0,), noisy=_others((0,))),
    Recipe('C', rec_C, 9011, zero=(), noisy=ALL),
    Recipe('Q', rec_Q, 9012, zero=(), noisy=ALL),
    Recipe('Q2', rec_Q2, 9013, zero=(), noisy=ALL),
] + [Recipe('N%d' % m, rec_N(m), 9020 + m) for m in N_LAST] + [
    Recipe('S', rec_S, 9014),
    Recipe('S2', rec_S2, 9015),
    Recipe('T', rec_T, 9016),
    Recipe('T2', rec_T2, 9017),
]
# the recipes the two restatements were checked on at the 4-day cadence
DEFINED_4D = [r for r in DEFINED_16D if r.name in ('B', 'H', 'I', 'J', 'K', 'M', 'M2', 'M3')]
ROUNDING = [
    Recipe('A', rec_A, 9101),
    Recipe('E', rec_E, 9102),
    Recipe('F', rec_F, 9103),
    Recipe('G', rec_G, 9104),
]
TMASK_BANDS = (1, 4)  # green, swir1 (the default)

DEFINED = {'16d': DEFINED_16D, '4d': DEFINED_4D}


def batch(recipes, cadence):
    """(dates [n], spectra [7][P][n] int16, qa [P][n] uint16) of the recipes, in list order"""
    d = DATES[cadence]
    made = [r.make(d, cadence) for r in recipes]
    return d.copy(), np.stack([m[0] for m in made], axis=1), np.stack([m[1] for m in made], axis=0)


def defined(cadence):
    return batch(DEFINED[cadence], cadence)


def rounding_decided(cadence):
    return batch(ROUNDING, cadence)


def names(recipes):
    return [r.name for r in recipes]


def index(recipes, name):
    return names(recipes).index(name)


def standard_filtered(d, s_px, q_px):
    """(dates [k], observations [7][k], mask [n]) of one pixel as the reference's standard
    procedure hands them to adjusted_variogram: dates sorted, thermal converted to Celsius x 100,
    the standard filter applied (mask: in sorted-date order) -- from oracle/ccd_ref.py alone"""
    import ccd_ref
    p = ccd_ref.get_params()
    o = ccd_ref.argsort(d, p)
    dates, obs, q = d[o], s_px[:, o].copy(), ccd_ref.unpackqa(q_px[o], p)
    obs[p.THERMAL_IDX] = ccd_ref.kelvin_to_celsius(obs[p.THERMAL_IDX])
    mask = ccd_ref.standard_procedure_filter(obs, q, dates, p)
    return dates[mask], obs[:, mask], mask
