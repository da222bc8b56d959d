"""ccdc.products -- the annual change and land-cover product rasters made from the segment table:
what LCMAP's users receive (Spark-free; no counterpart module in the reference, whose ecosystem makes
them in a separate product generator, lcmap-gaia, that is not pinned here -- parity with it is not
claimed, and where its choice is not certain it is a parameter: bot, mag_bands, cover, labels).

Per pixel and product date (normally the 1 July of each year, ``synthetic.annual_dates``): time of
spectral change (sctime), change magnitude (scmag), time since last change (sclast), spectral
stability period (scstab), model quality (scmqa), primary and secondary land cover with their
confidences (lcpri, lcsec, lcpconf, lcsconf) and annual land-cover change (lcachg).
include/ccdgpu.h states the rule; the evaluation runs on the device (ccd_products.hip through
``ccdgpu.Context.products`` / ``products_rows``); there is no CPU path.

    keys, prod = products.annual(segment_table, synthetic.annual_dates(1985, 2017))
    rasters = products.rasters(keys, prod['sctime'][0])    # {(cx, cy): uint16 [100][100]} of 1985
"""
import numpy as np
import pyarrow.compute as pc

from ccdc import synthetic


def _context(context):
    import ccdgpu
    return context or ccdgpu.default_context()


def _rfrawp_column(segments, order):
    """The table's rfrawp column as float32 [n_rows][n_classes] in the rows' order, NaN where it is
    null; None when the table has no such column or it holds no prediction."""
    if 'rfrawp' not in segments.column_names or segments.num_rows == 0:
        return None
    col = segments['rfrawp'].combine_chunks()
    valid = pc.is_valid(col).to_numpy(zero_copy_only=False)
    if not valid.any():
        return None
    flat = np.asarray(col.flatten().to_numpy(zero_copy_only=False), dtype=np.float32)
    n_valid = int(valid.sum())
    if flat.shape[0] % n_valid:
        raise ValueError('rfrawp must hold the same number of classes in every row')
    raw = np.full((segments.num_rows, flat.shape[0] // n_valid), np.nan, dtype=np.float32)
    raw[valid] = flat.reshape(n_valid, -1)
    return raw[order]


def annual(segments, dates, rfrawp=None, labels=None, cover='extend', bot=None, mag_bands=None, want=None, context=None):
    """Product rasters of every pixel of an Arrow segment table at ``dates`` (ordinals, dates or ISO
    strings, in the order the annual change is to follow): (keys [n_pixels][4] = cx, cy, px, py,
    {name: array [n_dates][n_pixels]}).  rfrawp: float32 [n_rows][n_classes] aligned with the
    table's rows; by default the table's own rfrawp column when ``randomforest.join`` (or
    ``classify_chips_tables``) has put one there -- without either only the change products are made.
    labels: the product value of each class (default k + 1)."""
    keys, offsets, rows, order = synthetic.rows_order_from_table(segments)
    if rfrawp is None:
        raw = _rfrawp_column(segments, order)
    else:
        raw = np.asarray(rfrawp, dtype=np.float32)
        if raw.ndim != 2 or raw.shape[0] != segments.num_rows:
            raise ValueError('rfrawp must be [%d][n_classes], got %r' % (segments.num_rows, raw.shape))
        raw = raw[order]
    prod = _context(context).products(offsets, rows, synthetic.ordinals(dates), rfrawp=raw, labels=labels, cover=cover, bot=bot,
                                      mag_bands=mag_bands, want=want)
    return keys, prod


def rasters(keys, plane, width=100):
    """One date's plane [n_pixels] scattered into chip rasters: {(cx, cy): [width][width]} with the
    pixel (px, py) at row (cy - py) / 30, column (px - cx) / 30; cells no pixel fills are 0."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 4)
    plane = np.asarray(plane).reshape(-1)
    if plane.shape[0] != keys.shape[0]:
        raise ValueError('the plane has %d pixels, the keys %d' % (plane.shape[0], keys.shape[0]))
    col, row = (keys[:, 2] - keys[:, 0]) // 30, (keys[:, 1] - keys[:, 3]) // 30
    if (((keys[:, 2] - keys[:, 0]) % 30 != 0) | ((keys[:, 1] - keys[:, 3]) % 30 != 0) | (col < 0) | (col >= width) |
            (row < 0) | (row >= width)).any():
        raise ValueError('a pixel lies outside its %d x %d chip' % (width, width))
    out = {}
    chips, first, inverse = np.unique(keys[:, :2], axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    for k in np.argsort(first, kind='stable'):
        sel = inverse == k
        r = np.zeros((width, width), dtype=plane.dtype)
        r[row[sel], col[sel]] = plane[sel]
        out[(int(chips[k, 0]), int(chips[k, 1]))] = r
    return out


def annual_chips(chips, dates, aux_of=None, forest=None, params=None, context=None, labels=None, cover='extend', bot=None,
                 mag_bands=None, want=None, symmetric=True):
    """Detection straight from chipmunk chips (``pyccd.detect_chips``' input) with each chip's product
    rasters made right behind its batch's detection, from the segments still on the device
    (``Context.products_rows``).  With a forest and aux_of(cx, cy) -- the chip's [n_pix][5] aux values
    (dem, aspect, slope, mpw, posidex), pixels in row-major order -- the batch's rows are classified
    there first (``Context.classify_rows``) and the cover products are made too.  Returns
    [((cx, cy), {name: array [n_dates][n_pix]})] in first-seen order; a plane of a 100 x 100 chip,
    reshaped (100, 100), is its raster."""
    import ccdgpu
    from ccdc import pyccd
    ctx = _context(context)
    classify = forest is not None and aux_of is not None
    if classify:
        ctx.set_forest(forest)
    at = synthetic.ordinals(dates)
    state = {}

    def on_batch(ctx, keys, n_pix):
        aux = np.concatenate([np.asarray(aux_of(cx, cy), dtype=np.float64).reshape(n_pix, 5) for cx, cy in keys])
        state['raw'], state['at'] = ctx.classify_rows(aux), 0

    out = []
    for ctx, c, (cx, cy), _, n_pix in pyccd._run_chips(chips, params, ctx, symmetric, on_batch=on_batch if classify else None):
        bad = ctx.fetch(c).error_pixel if ctx.qa_error else -1  # (the batch had one: is it this chip's?)
        if bad >= 0:
            raise ccdgpu.QAValueError('unsupported QA value at pixel %d of chip (%d, %d)' % (bad, cx, cy))
        raw = None
        if classify:  # the batch's rows are chip-major
            a, n = state['at'], ctx.chip_row_count(c)
            raw, state['at'] = state['raw'][a:a + n], a + n
        out.append(((cx, cy), ctx.products_rows(c, at, rfrawp=raw, labels=labels, cover=cover, bot=bot, mag_bands=mag_bands,
                                                want=want)))
    return out
