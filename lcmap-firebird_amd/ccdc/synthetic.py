"""ccdc.synthetic -- band values predicted from the segment models: what the segment table exists
for (Spark-free; no counterpart module in the reference, whose consumers evaluate the table's
models themselves with lcmap-pyccd's ``ccd.models.lasso.predict`` over ``coefficient_matrix``).

A segment row carries, per band, an intercept and seven harmonic coefficients.  The modelled
surface reflectance of a pixel at a date -- the 1 July annual composites, "synthetic Landsat"
images, the residual of an observation against its model -- is the row's model evaluated at that
date.  include/ccdgpu.h states the rule (basis, which row a date takes, the order of the sum, the
output types); the evaluation runs on the device (ccd_predict.hip through
``ccdgpu.Context.predict`` / ``predict_rows``); there is no CPU path.

    keys, values, seg_index = synthetic.predict(segment_table, synthetic.annual_dates(1985, 2017))
    # values [7][n_pixels][33] float32, NaN where no segment covers the date
"""
from datetime import date

import numpy as np
import pyarrow.compute as pc

from ccdc import sink

_DAY_COLS = ('sday', 'eday', 'bday')


def ordinals(dates):
    """Proleptic ordinals (int64) of ``dates``: ordinals, ``datetime.date`` objects or ISO
    'YYYY-MM-DD' strings (one kind per call)."""
    if isinstance(dates, np.ndarray) and dates.dtype.kind in 'iu':
        return np.ascontiguousarray(dates, dtype=np.int64).reshape(-1)
    items = list(dates)
    if not items:
        return np.zeros(0, dtype=np.int64)
    if isinstance(items[0], str):
        return _iso_ordinals(np.asarray(items, dtype=str))
    if isinstance(items[0], date):
        return np.asarray([d.toordinal() for d in items], dtype=np.int64)
    return np.asarray(items, dtype=np.int64).reshape(-1)


def _iso_ordinals(iso):
    """'YYYY-MM-DD' strings -> proleptic ordinals (the inverse of sink.iso_days)."""
    return (np.asarray(iso, dtype='datetime64[D]') - sink._EPOCH).astype(np.int64) + 1


def annual_dates(first_year, last_year, month=7, day=1):
    """The ordinals of (month, day) of every year first_year .. last_year: the dates of the annual
    composites (1 July by default)."""
    return np.asarray([date(y, month, day).toordinal() for y in range(int(first_year), int(last_year) + 1)], dtype=np.int64)


def _column(t, name, dtype, fill=0):
    """A column as a numpy array, nulls replaced by ``fill``."""
    col = t[name].combine_chunks() if t.num_rows else t[name]
    return np.asarray(pc.fill_null(col, fill).to_numpy(zero_copy_only=False), dtype=dtype)


def rows_from_table(segments):
    """The Arrow segment table of ccdc.sink (one chip's, or several concatenated) ->
    (keys int32 [n_pixels][4] = cx, cy, px, py in first-appearance order, row_offsets int64
    [n_pixels + 1], rows abi.ROW_DTYPE [n_rows]): a pixel's rows together, in table order.  ISO days
    become ordinals (a null bday 0); a null chprob marks pyccd.default's row, has_model 0, whose null
    columns become 0."""
    return rows_order_from_table(segments)[:3]


def rows_order_from_table(segments):
    """``rows_from_table`` with, fourth, the table row each returned row came from (int64 [n_rows]):
    what brings a column of the table that is not part of the rows -- rfrawp -- into their order."""
    from ccdgpu import abi
    n = segments.num_rows
    rows = np.zeros(n, dtype=abi.ROW_DTYPE)
    if n == 0:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(1, dtype=np.int64), rows, np.zeros(0, dtype=np.int64)
    key = np.stack([_column(segments, k, np.int32) for k in ('cx', 'cy', 'px', 'py')], axis=1)
    rows['px'], rows['py'] = key[:, 2], key[:, 3]
    for k in _DAY_COLS:
        iso = pc.fill_null(segments[k], '0001-01-01').to_numpy(zero_copy_only=False).astype(str)
        days = _iso_ordinals(iso)
        days[~pc.is_valid(segments[k]).to_numpy(zero_copy_only=False)] = 0
        rows[k] = days
    valid = pc.is_valid(segments['chprob']).to_numpy(zero_copy_only=False)
    rows['has_model'] = valid
    rows['chprob'] = _column(segments, 'chprob', np.float32)
    rows['curqa'] = _column(segments, 'curqa', np.int32)
    for b, pre in enumerate(sink.BAND_PREFIX):
        rows['mag'][:, b] = _column(segments, pre + 'mag', np.float32)
        rows['rmse'][:, b] = _column(segments, pre + 'rmse', np.float32)
        rows['intercept'][:, b] = _column(segments, pre + 'int', np.float32)
        col = segments[pre + 'coef'].combine_chunks()
        has = pc.is_valid(col).to_numpy(zero_copy_only=False)
        flat = np.asarray(col.flatten().to_numpy(zero_copy_only=False), dtype=np.float32)
        if flat.shape[0] != 7 * int(has.sum()):
            raise ValueError('%scoef must hold 7 coefficients per row' % pre)
        rows['coef'][has, b, :] = flat.reshape(-1, 7)
    # pixels in first-appearance order, each pixel's rows together in table order
    uniq, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(uniq.shape[0], dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(uniq.shape[0])
    pixel = rank[inverse.reshape(-1)]
    order = np.argsort(pixel, kind='stable')
    offsets = np.concatenate([[0], np.cumsum(np.bincount(pixel, minlength=uniq.shape[0]))]).astype(np.int64)
    return key[np.sort(first)], offsets, rows[order], order


def _context(context):
    import ccdgpu
    return context or ccdgpu.default_context()


def predict(segments, dates, cover='span', dtype='float32', avg_days_yr=365.2425, context=None):
    """Band values of every pixel of an Arrow segment table at ``dates`` (ordinals, dates or ISO
    strings, any order): (keys [n_pixels][4], values [7][n_pixels][n_dates] float32 or int16,
    seg_index int32 [n_pixels][n_dates]).  cover 'span': a date takes the segment whose
    sday .. eday holds it; 'extend': the last segment begun by then, so the model holds through
    the gap after a break and after the last segment.  No segment: NaN / -9999, seg_index -1."""
    keys, offsets, rows = rows_from_table(segments)
    values, idx = _context(context).predict(offsets, rows, ordinals(dates), avg_days_yr=avg_days_yr, cover=cover, dtype=dtype)
    return keys, values, idx


def predict_chips(chips, dates_of=None, params=None, context=None, cover='span', dtype='float32', avg_days_yr=365.2425,
                  symmetric=True):
    """Detection straight from chipmunk chips (``pyccd.detect_chips``' input) with each chip's
    band values predicted right behind its batch's detection, from the segments still on the
    device (``Context.predict_rows``).  dates_of(cx, cy, dates) gives the dates to predict a chip
    at (ordinals, dates or ISO strings); by default the chip's own acquisition dates, in input
    order, so ``spectra - values`` are the residuals.  Returns [((cx, cy), dates int64 [n],
    values [7][n_pix][n], seg_index [n_pix][n])] in first-seen order."""
    import ccdgpu
    from ccdc import pyccd
    out = []
    for ctx, c, (cx, cy), dates, n_pix in pyccd._run_chips(chips, params, _context(context), symmetric):
        bad = ctx.fetch(c).error_pixel if ctx.qa_error else -1  # (the batch had one: is it this chip's?)
        if bad >= 0:
            raise ccdgpu.QAValueError('unsupported QA value at pixel %d of chip (%d, %d)' % (bad, cx, cy))
        at = ordinals(dates if dates_of is None else dates_of(cx, cy, dates))
        values, idx = ctx.predict_rows(c, at, avg_days_yr=avg_days_yr, cover=cover, dtype=dtype)
        out.append(((cx, cy), at, values, idx))
    return out
