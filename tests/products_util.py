"""numpy restatement of the product rule of include/ccdgpu.h (the rule of ccd_products.hip), written
twice: ``products`` vectorised (per row once, then per pixel over rows x dates), and ``products_loop``
one value at a time, the rule's sentences word for word.  Its own year window comes from
datetime.date.  numpy and Python floats round every product, sum, quotient and square root on its
own, as the kernel (built without FMA contraction) does, so the restatement is bit-equal to the
device.  Also a generator of row tables and rfrawp matrices that reach every branch of the rule."""
from datetime import date
from types import SimpleNamespace

import numpy as np

import predict_util as pu
from ccdgpu import abi

NAMES = tuple(n for n, _ in abi.PRODUCTS)
NAN32 = pu.NAN32
# rows per pixel of the generated tables: none, pyccd.default's row, 1, 2, 13 and 70
COUNTS = (0, 'd', 1, 2, 13, 70)
N_CLASSES = (1, 2, 9, 32)
MIN = np.int64(-1) << 40  # below every day


def params(bot=abi.PRODUCT_BOT, mag_bands=abi.PRODUCT_MAG_BANDS, cover=abi.COVER_EXTEND, n_classes=0, labels=None):
    """The rule's parameters with their defaults (labels: k + 1)."""
    lab = np.arange(1, 33, dtype=np.uint8) if labels is None else np.asarray(labels, dtype=np.uint8)
    return SimpleNamespace(bot=int(bot), mag_bands=int(mag_bands), cover=int(cover), n_classes=int(n_classes), labels=lab)


def year_window(dates):
    """(a, b): the ordinals of 1 January of each date's year and of the next, from datetime.date."""
    a, b = [], []
    for t in np.asarray(dates, dtype=np.int64).tolist():
        y = date.fromordinal(t).year
        a.append(date(y, 1, 1).toordinal())
        b.append(date(y + 1, 1, 1).toordinal() if y < date.max.year else date.max.toordinal() + 1)
    return np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)


def _empty(n_dates, n_pix, names):
    return {n: np.zeros((n_dates, n_pix), dtype=abi.PRODUCT_DTYPES[n]) for n in names}


def _names(rfrawp):
    return NAMES if rfrawp is not None else abi.CHANGE_PRODUCTS


# ---- vectorised -------------------------------------------------------------------------------------
def records(rows, rfrawp, par):
    """What the products need of each row, once per row: model, break, scmag, clamped curqa, and --
    with an rfrawp -- defined, label1, label2, conf1, conf2."""
    r = SimpleNamespace()
    r.model = rows['has_model'] != 0
    r.brk = r.model & (rows['chprob'] == np.float32(1.0)) & (rows['bday'] >= 1)
    s = np.zeros(rows.shape[0], dtype=np.float64)
    with np.errstate(all='ignore'):
        for b in range(abi.NBANDS):
            if (par.mag_bands >> b) & 1:
                m = rows['mag'][:, b].astype(np.float64)
                s = s + m * m
        r.scmag = np.sqrt(s).astype(np.float32)
    r.scmag[np.isnan(r.scmag)] = NAN32
    r.curqa = np.clip(rows['curqa'], 0, 255).astype(np.uint8)
    if rfrawp is None:
        return r
    n, nc = rows.shape[0], par.n_classes
    raw = np.asarray(rfrawp, dtype=np.float32)[:, :nc].astype(np.float64)
    with np.errstate(all='ignore'):
        S = np.zeros(n, dtype=np.float64)
        for k in range(nc):
            S = S + raw[:, k]
        r.defined = ~np.isnan(raw).any(axis=1) & np.isfinite(S) & (S > 0.0)
        at = np.arange(n)
        safe = np.where(r.defined[:, None], raw, 0.0)
        i1 = np.argmax(safe, axis=1)  # the first of the largest
        rest = safe.copy()
        rest[at, i1] = -np.inf
        i2 = np.argmax(rest, axis=1)
        Ss = np.where(r.defined, S, 1.0)
        c1 = np.clip(np.rint(100.0 * safe[at, i1] / Ss), 0.0, 100.0)
        c2 = np.clip(np.rint(100.0 * safe[at, i2] / Ss), 0.0, 100.0)
    two = r.defined & (nc >= 2)
    r.label1 = np.where(r.defined, par.labels[i1], 0).astype(np.uint8)
    r.label2 = np.where(two, par.labels[i2], 0).astype(np.uint8)
    r.conf1 = np.where(r.defined, c1, 0).astype(np.uint8)
    r.conf2 = np.where(two, c2, 0).astype(np.uint8)
    return r


def _first(ok):
    """(index of the first True along axis 0, whether there is one)."""
    return np.argmax(ok, axis=0), ok.any(axis=0)


def products(offsets, rows, dates, rfrawp=None, par=None):
    """{name: [n_dates][n_pix]}: the change products, and the cover products when rfrawp is given."""
    par = par or params()
    t = np.asarray(dates, dtype=np.int64)
    n_pix, n_dates = len(offsets) - 1, t.shape[0]
    out = _empty(n_dates, n_pix, _names(rfrawp))
    if n_dates == 0 or n_pix == 0:
        return out
    a, b = year_window(t)
    rec = records(rows, rfrawp, par)
    taken = pu.select(offsets, rows, t, par.cover)
    t, a, b = t[None, :], a[None, :], b[None, :]
    for p in range(n_pix):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        none = np.where(t[0] >= par.bot, np.minimum(t[0] - par.bot, 65535), 0)
        if hi == lo:
            out['scstab'][:, p] = none
            continue
        sl = slice(lo, hi)
        sday, eday, bday = (rows[k][sl].astype(np.int64)[:, None] for k in ('sday', 'eday', 'bday'))
        model, brk = rec.model[sl][:, None], rec.brk[sl][:, None]
        j, any_ = _first(brk & (a <= bday) & (bday < b))
        out['sctime'][:, p] = np.where(any_, bday[j, 0] - a[0] + 1, 0)
        out['scmag'][:, p] = np.where(any_, rec.scmag[sl][j], np.float32(0.0))
        g_last = np.where(brk & (bday <= t), bday, MIN).max(axis=0)
        out['sclast'][:, p] = np.where(g_last > MIN, np.minimum(t[0] - g_last, 65535), 0)
        g_stab = np.maximum(np.where(model & (sday <= t), sday, MIN).max(axis=0), g_last)
        out['scstab'][:, p] = np.where(g_stab > MIN, np.minimum(t[0] - g_stab, 65535), none)
        j, any_ = _first(model & (sday <= t) & (t <= eday))
        out['scmqa'][:, p] = np.where(any_, rec.curqa[sl][j], 0)
        if rfrawp is None:
            continue
        j = np.maximum(taken[p], 0)
        ok = (taken[p] >= 0) & rec.defined[sl][j]
        pri = np.where(ok, rec.label1[sl][j], 0)
        out['lcpri'][:, p] = pri
        out['lcsec'][:, p] = np.where(ok, rec.label2[sl][j], 0)
        out['lcpconf'][:, p] = np.where(ok, rec.conf1[sl][j], 0)
        out['lcsconf'][:, p] = np.where(ok, rec.conf2[sl][j], 0)
        q, c = pri[:-1].astype(np.int64), pri[1:].astype(np.int64)
        out['lcachg'][1:, p] = np.where((q != 0) & (c != 0) & (q != c), q * 256 + c, 0)
    return out


# ---- one value at a time --------------------------------------------------------------------------
def _cover_of(raw, par):
    """(lcpri, lcsec, lcpconf, lcsconf) of one rfrawp row, the rule's sentences in order."""
    vals = [float(np.float64(x)) for x in raw[:par.n_classes]]
    if any(v != v for v in vals):
        return 0, 0, 0, 0
    S = 0.0
    for v in vals:
        S = S + v
    if not (np.isfinite(S) and S > 0.0):
        return 0, 0, 0, 0
    i1 = None
    for k, v in enumerate(vals):
        if i1 is None or v > vals[i1]:
            i1 = k
    i2 = None
    for k, v in enumerate(vals):
        if k != i1 and (i2 is None or v > vals[i2]):
            i2 = k

    def conf(i):
        return int(min(max(np.rint(100.0 * vals[i] / S), 0.0), 100.0))
    if i2 is None:
        return int(par.labels[i1]), 0, conf(i1), 0
    return int(par.labels[i1]), int(par.labels[i2]), conf(i1), conf(i2)


def _scmag_of(mag, par):
    s = 0.0
    with np.errstate(all='ignore'):
        for b in range(abi.NBANDS):
            if (par.mag_bands >> b) & 1:
                m = np.float64(mag[b])
                s = s + m * m
        v = np.float32(np.sqrt(np.float64(s)))
    return NAN32 if np.isnan(v) else v


def products_loop(offsets, rows, dates, rfrawp=None, par=None):
    """``products`` one pixel, date and row at a time."""
    par = par or params()
    dates = np.asarray(dates, dtype=np.int64).tolist()
    n_pix = len(offsets) - 1
    out = _empty(len(dates), n_pix, _names(rfrawp))
    a_of, b_of = (x.tolist() for x in year_window(dates))
    taken = pu.select_loop(offsets, rows, dates, par.cover)
    for p in range(n_pix):
        r = rows[offsets[p]:offsets[p + 1]]
        n = r.shape[0]
        sday, eday, bday, curqa = (r[k].tolist() for k in ('sday', 'eday', 'bday', 'curqa'))
        model = [int(h) != 0 for h in r['has_model']]
        brk = [model[j] and r['chprob'][j] == np.float32(1.0) and bday[j] >= 1 for j in range(n)]
        prev = 0
        for i, t in enumerate(dates):
            a, b = a_of[i], b_of[i]
            for j in range(n):  # the first break of the date's year
                if brk[j] and a <= bday[j] < b:
                    out['sctime'][i, p] = bday[j] - a + 1
                    out['scmag'][i, p] = _scmag_of(r['mag'][j], par)
                    break
            last = [bday[j] for j in range(n) if brk[j] and bday[j] <= t]
            if last:
                out['sclast'][i, p] = min(t - max(last), 65535)
            stab = last + [sday[j] for j in range(n) if model[j] and sday[j] <= t]
            if stab:
                out['scstab'][i, p] = min(t - max(stab), 65535)
            elif t >= par.bot:
                out['scstab'][i, p] = min(t - par.bot, 65535)
            for j in range(n):  # the first model whose span holds the date
                if model[j] and sday[j] <= t <= eday[j]:
                    out['scmqa'][i, p] = min(max(curqa[j], 0), 255)
                    break
            if rfrawp is None:
                continue
            pri = 0
            if taken[p, i] >= 0:
                pri, sec, c1, c2 = _cover_of(rfrawp[offsets[p] + taken[p, i]], par)
                out['lcpri'][i, p], out['lcsec'][i, p], out['lcpconf'][i, p], out['lcsconf'][i, p] = pri, sec, c1, c2
            if i > 0 and prev != 0 and pri != 0 and prev != pri:
                out['lcachg'][i, p] = prev * 256 + pri
            prev = pri
    return out


# ---- generated tables -------------------------------------------------------------------------------
def product_dates(n_dates):
    """0, 1, 2 or 33 product dates, 1 Julys: 1990; 1995 then 1990; 1980 .. 2011 shuffled with one of
    them twice (1980 and 1981 lie before the default beginning of time)."""
    if n_dates == 0:
        return np.zeros(0, dtype=np.int64)
    if n_dates == 1:
        return np.asarray([date(1990, 7, 1).toordinal()], dtype=np.int64)
    if n_dates == 2:
        return np.asarray([date(1995, 7, 1).toordinal(), date(1990, 7, 1).toordinal()], dtype=np.int64)
    assert n_dates == 33
    d = np.asarray([date(y, 7, 1).toordinal() for y in range(1980, 2012)] + [date(1999, 7, 1).toordinal()], dtype=np.int64)
    return d[np.random.default_rng(33).permutation(33)]


def table(seed, n_pix, dates):
    """(row_offsets, rows) on predict_util.random_table's shapes with COUNTS rows per pixel, made to
    reach the change products' branches: chprob exactly 1.0 on about half the rows, 0.0, 0.5 and NaN on
    others; bday in the year of a product date, on its 1 January, its 31 December, the date itself,
    0, or as generated; two breaks in one year on some pixels; some NaN mag values and some curqa
    above 255 and below 0.  (random_table shuffles the rows of every third pixel.)"""
    off, rows = pu.random_table(seed, n_pix, counts=COUNTS)
    rng = np.random.default_rng(seed + 1000)
    n = rows.shape[0]
    model = rows['has_model'] != 0
    chprob = np.where(rng.random(n) < 0.5, 1.0, rng.choice(np.float32([0.0, 0.5, np.nan]), n)).astype(np.float32)
    rows['chprob'] = np.where(model, chprob, rows['chprob'])
    pool = np.asarray(dates, dtype=np.int64) if len(dates) else np.asarray([date(1990, 7, 1).toordinal()], dtype=np.int64)
    t = rng.choice(pool, n)
    a, b = year_window(t)
    mode = rng.integers(0, 6, n)
    bday = np.select([mode == 0, mode == 1, mode == 2, mode == 3, mode == 4],
                     [a + rng.integers(0, 365, n), a, b - 1, t, np.zeros(n, dtype=np.int64)], rows['bday'].astype(np.int64))
    rows['bday'] = np.where(model, bday, rows['bday'])
    for p in range(0, n_pix, 4):  # two breaks in one year: the first in table order is the year's
        lo, hi = int(off[p]), int(off[p + 1])
        if hi - lo >= 2 and model[lo] and model[lo + 1]:
            rows['chprob'][lo:lo + 2] = 1.0
            rows['bday'][lo], rows['bday'][lo + 1] = a[lo] + 200, a[lo] + 100
    rows['mag'][model & (rng.random(n) < 0.05), 3] = np.nan
    rows['curqa'] = np.where(model, rng.choice([0, 4, 8, 24, 255, 256, 300, -5], n), rows['curqa'])
    return off, rows


def rfrawp_for(seed, rows, n_classes):
    """float32 [n_rows][n_classes] like a forest's raw predictions (non-negative, summing to 500), NaN
    for rows without a model, and with: exact ties (of all classes, and of the largest at later
    indices), quotients on a half (1 : 7 and 3 : 5), a negative secondary value, a NaN row, an
    all-zero row, a row with an infinity."""
    rng = np.random.default_rng(seed + 2000)
    n = rows.shape[0]
    raw = rng.integers(0, 40, (n, n_classes)).astype(np.float32)
    raw *= np.float32(500.0) / np.maximum(raw.sum(axis=1, keepdims=True), 1)
    kind = rng.integers(0, 16, n)
    raw[kind == 0] = 7.0
    if n_classes >= 2:
        raw[kind == 1] = 0.0
        raw[kind == 1, -1] = raw[kind == 1, n_classes // 2] = 11.0
        raw[kind == 2] = 0.0
        raw[kind == 2, 0], raw[kind == 2, -1] = 1.0, 7.0
        raw[kind == 3] = 0.0
        raw[kind == 3, 0], raw[kind == 3, 1] = 5.0, 3.0
        raw[kind == 4, 0], raw[kind == 4, 1:] = 9.0, -0.25
    raw[kind == 5, 0] = np.nan
    raw[kind == 6] = 0.0
    raw[kind == 7, -1] = np.inf
    raw[rows['has_model'] == 0] = np.nan
    return np.ascontiguousarray(raw, dtype=np.float32)


def case(seed, n_pix, n_dates, n_classes):
    """(row_offsets, rows, dates, rfrawp) of one generated case."""
    dates = product_dates(n_dates)
    off, rows = table(seed, n_pix, dates)
    return off, rows, dates, rfrawp_for(seed, rows, n_classes)


N_PIX = (0, 1, 3, 63, 64, 65, 100, 257)
N_DATES = (0, 1, 2, 33)


def grid():
    """The cases of the exactness test: every (n_pix, n_dates), the class counts and the two covers
    going round; (seed, n_pix, n_dates, n_classes, cover)."""
    out = []
    for i, n_pix in enumerate(N_PIX):
        for j, n_dates in enumerate(N_DATES):
            k = i * len(N_DATES) + j
            out.append((100 + k, n_pix, n_dates, N_CLASSES[(i + j) % 4], (abi.COVER_SPAN, abi.COVER_EXTEND)[(i + j // 2) % 2]))
    return out


def sqrt_mags(seed, n):
    """float32 [n][7] magnitudes whose sums of squares, under the masks of SQRT_MASKS, are the s of the
    square-root test: one-band sums (perfect squares of float32 values -- ordinary, tiny down to the
    denormals, huge up to FLT_MAX) in band 0; in bands 1 and 2 a value and a second one whose square
    is 0.5 to 4 units in the last place of the first's square, so that the two-band sum is a perfect
    square's double neighbour (or, on a tie, the square itself); bands 3 .. 6 random, a general s."""
    rng = np.random.default_rng(seed)
    mag = np.zeros((n, 7), dtype=np.float32)
    scale = np.float32(10.0) ** rng.integers(-44, 39, n).astype(np.float32)
    with np.errstate(over='ignore', under='ignore'):
        mag[:, 0] = (rng.normal(0, 1, n).astype(np.float32) * scale).astype(np.float32)
    mag[:8, 0] = [0.0, 1.0, 3.0, np.float32(3.4028235e38), np.float32(1e-45), np.float32(1.1754944e-38), 4096.0, np.inf]
    m1 = (rng.random(n) * 4000 + 1).astype(np.float32)
    sq = m1.astype(np.float64) ** 2
    mag[:, 1] = m1
    mag[:, 2] = np.sqrt(np.spacing(sq) * rng.choice([0.5, 1.0, 1.5, 2.0, 4.0], n)).astype(np.float32)
    mag[:, 3:] = rng.normal(0, 300, (n, 4)).astype(np.float32)
    return mag


SQRT_MASKS = (0x01, 0x02, 0x04, 0x06, 0x78, 0x7F)
