"""numpy restatement of the prediction rule of include/ccdgpu.h (the rule of ccd_predict.hip):
which row a date takes, written as plain comparisons; the left-to-right sum over a basis that is
passed in; the two output conversions; and a generator of random row tables.  numpy rounds every
product and every sum on its own, as the kernel (built without FMA contraction) does, so given the
device's basis (Context.coefficient_matrix) the restatement is bit-equal to the device."""
import numpy as np

from ccdgpu import abi

SPAN, EXTEND = abi.COVER_SPAN, abi.COVER_EXTEND
F32, I16 = abi.PREDICT_F32, abi.PREDICT_I16
NAN32 = np.frombuffer(np.uint32(0x7fc00000).tobytes(), dtype=np.float32)[0]

# rows per pixel of the generated tables: none; only pyccd.default's row ('d'); 1, 2, 13; the
# kernel's per-block model cache, one more, two caches and one more; 70 (> 64).
CACHE = abi.PREDICT_CACHE_ROWS
COUNTS = (0, 'd', 1, 2, 13, CACHE, CACHE + 1, 2 * CACHE + 1, 70)


def basis(dates, avg_days_yr=365.2425):
    """The seven lines of the rule with numpy's own cos / sin: [n_dates][7] float64."""
    t = np.asarray(dates, dtype=np.int64)
    w = 2.0 * np.pi / avg_days_yr
    w12 = w * t.astype(np.float64)
    w34 = 2.0 * w12
    w56 = 3.0 * w12
    return np.stack([t.astype(np.float64), np.cos(w12), np.sin(w12), np.cos(w34), np.sin(w34), np.cos(w56), np.sin(w56)], axis=1)


def select(offsets, rows, dates, cover):
    """seg_index int32 [n_pix][n_dates]: the taken row's index within its pixel, or -1."""
    t = np.asarray(dates, dtype=np.int64)[None, :]
    n_pix = len(offsets) - 1
    out = np.full((n_pix, t.shape[1]), -1, dtype=np.int32)
    for p in range(n_pix):
        r = rows[offsets[p]:offsets[p + 1]]
        if r.shape[0] == 0 or t.shape[1] == 0:
            continue
        sday, eday = r['sday'].astype(np.int64)[:, None], r['eday'].astype(np.int64)[:, None]
        has = (r['has_model'] != 0)[:, None]
        if cover == SPAN:  # the first row in table order with sday <= t <= eday
            ok = has & (sday <= t) & (t <= eday)
            j = np.argmax(ok, axis=0)
        else:              # the greatest sday <= t, ties going to the later row
            ok = has & (sday <= t)
            key = np.where(ok, sday, np.int64(-1) << 40)
            j = r.shape[0] - 1 - np.argmax(key[::-1], axis=0)
        out[p] = np.where(ok.any(axis=0), j, -1)
    return out


def select_loop(offsets, rows, dates, cover):
    """``select`` one value at a time, the rule's sentences word for word."""
    out = np.full((len(offsets) - 1, len(dates)), -1, dtype=np.int32)
    for p in range(len(offsets) - 1):
        r = rows[offsets[p]:offsets[p + 1]]
        has, sday, eday = r['has_model'].tolist(), r['sday'].tolist(), r['eday'].tolist()
        for i, t in enumerate(np.asarray(dates).tolist()):
            taken = -1
            for j in range(len(has)):
                if has[j] == 0 or not sday[j] <= t:
                    continue
                if cover == SPAN:
                    if t <= eday[j]:
                        taken = j
                        break
                elif taken < 0 or sday[j] >= sday[taken]:
                    taken = j
            out[p, i] = taken
    return out


def evaluate(offsets, rows, seg_index, B):
    """float64 [7][n_pix][n_dates]: v = intercept, then v = v + coef[k] * B[k] for k = 0 .. 6, of
    the taken rows' float32 values widened; NaN where no row is taken."""
    n_pix, n_dates = seg_index.shape
    v = np.full((abi.NBANDS, n_pix, n_dates), np.nan)
    if rows.shape[0] == 0 or n_dates == 0:
        return v
    none = seg_index < 0
    g = np.where(none, 0, np.asarray(offsets[:-1], dtype=np.int64)[:, None] + seg_index)
    g = np.minimum(g, rows.shape[0] - 1)
    for b in range(abi.NBANDS):
        a = rows['intercept'][:, b].astype(np.float64)[g]
        for k in range(7):
            a = a + rows['coef'][:, b, k].astype(np.float64)[g] * B[None, :, k]
        v[b] = np.where(none, np.nan, a)
    return v


def scale(offsets, rows, seg_index, dates):
    """S = |intercept| + |c0 t| + sum |ck| of every value: float64 [7][n_pix][n_dates] (0 where no
    row is taken)."""
    n_pix, n_dates = seg_index.shape
    none = seg_index < 0
    g = np.where(none, 0, np.asarray(offsets[:-1], dtype=np.int64)[:, None] + seg_index)
    g = np.minimum(g, max(rows.shape[0] - 1, 0))
    t = np.asarray(dates, dtype=np.float64)[None, :]
    s = np.zeros((abi.NBANDS, n_pix, n_dates))
    for b in range(abi.NBANDS):
        c = np.abs(rows['coef'][:, b, :].astype(np.float64))
        a = np.abs(rows['intercept'][:, b].astype(np.float64))[g] + c[:, 0][g] * t + c[:, 1:].sum(axis=1)[g]
        s[b] = np.where(none, 0.0, a)
    return s


def convert(v, seg_index, dtype):
    """The output conversions: float32 by round-to-nearest, a NaN value and the fill the quiet
    NaN; int16 by rint (halves to even) clamped, a NaN value and the fill -9999."""
    fill = np.isnan(v) | (seg_index < 0)[None]
    with np.errstate(over='ignore', invalid='ignore'):
        if dtype == F32:
            out = v.astype(np.float32)
            out[fill] = NAN32
            return out
        r = np.clip(np.rint(np.where(fill, 0.0, v)), -32768.0, 32767.0)
        return np.where(fill, abi.PREDICT_FILL_I16, r).astype(np.int16)


def predict(offsets, rows, dates, B, cover, dtype):
    """(values [7][n_pix][n_dates], seg_index) as Context.predict gives them."""
    idx = select(offsets, rows, dates, cover)
    return convert(evaluate(offsets, rows, idx, B), idx, dtype), idx


def random_table(seed, n_pix, counts=COUNTS):
    """(row_offsets int64 [n_pix + 1], rows abi.ROW_DTYPE): pixel p has counts[p % len(counts)]
    rows.  Spans do not overlap and have gaps (some of a single day, some spans a single day);
    every third pixel's rows are out of order; some pixels carry a has_model == 0 row whose span
    holds every date (never taken) and a row repeated with other coefficients (equal sday: span
    takes the first, extend the later)."""
    rng = np.random.default_rng(seed)
    per_pixel = []
    for p in range(n_pix):
        c = counts[p % len(counts)]
        n = 1 if c == 'd' else c
        r = np.zeros(n, dtype=abi.ROW_DTYPE)
        r['px'], r['py'] = 30 * p, -30 * p
        if c == 'd':
            r['sday'] = r['eday'] = r['bday'] = 1
        elif n:
            length = rng.integers(0, 400, n)
            gap = rng.integers(1, 90, n)
            sday = 724000 + int(rng.integers(0, 365)) + np.concatenate([[0], np.cumsum(length + gap)[:-1]])
            r['sday'], r['eday'], r['bday'] = sday, sday + length, sday + length + gap
            r['has_model'], r['curqa'] = 1, 8
            r['chprob'] = rng.random(n)
            r['intercept'] = rng.normal(0, 3000, (n, 7))
            r['coef'] = rng.normal(0, 500, (n, 7, 7))
            r['coef'][:, :, 0] = rng.normal(0, 2e-3, (n, 7))
            r['mag'], r['rmse'] = rng.normal(0, 100, (n, 7)), rng.random((n, 7)) * 100
            if n >= 2 and p % 4 == 1:  # the first row again, other coefficients, further down
                r[n - 1] = r[0]
                r['intercept'][n - 1] += 1000
            if n >= 2 and p % 5 == 2:  # a row without a model over every date
                r['has_model'][n // 2] = 0
                r['sday'][n // 2], r['eday'][n // 2] = 1, abi.PREDICT_MAX_DATE
            if p % 3 == 0:
                r = r[rng.permutation(n)]
        per_pixel.append(r)
    offsets = np.concatenate([[0], np.cumsum([r.shape[0] for r in per_pixel])]).astype(np.int64)
    rows = np.concatenate(per_pixel) if per_pixel else np.zeros(0, dtype=abi.ROW_DTYPE)
    return offsets, rows.astype(abi.ROW_DTYPE)


def edge_dates(rows):
    """Every sday, eday, sday - 1 and eday + 1 of the rows (within the accepted range), unique."""
    d = np.concatenate([rows['sday'], rows['eday'], rows['sday'] - 1, rows['eday'] + 1]).astype(np.int64)
    return np.unique(d[(d >= 1) & (d <= abi.PREDICT_MAX_DATE)])


def sample_dates(seed, rows, n_dates):
    """n_dates dates, shuffled and with repeats: drawn from edge_dates(rows) and from the years
    around the generated spans."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([edge_dates(rows), rng.integers(723000, 790000, 64)])
    return rng.choice(pool, n_dates, replace=True).astype(np.int64)
