"""Prediction of band values on the HIP path (ccd_predict.hip through ccdgpu.Context.predict /
predict_rows / coefficient_matrix) against the numpy restatement of tests/predict_util.py.  The
rule fixes every comparison and the order of every product and sum, so given the device's own basis
the comparisons are exact (bytes); only the basis itself (the device's cos / sin against numpy's)
and what follows from it are compared within bounds."""
import ctypes
import os
from datetime import date

import numpy as np
import pytest

import ccd_ref
import ccdgpu
import predict_util as pu
from ccdgpu import abi, synth
from ccdc import sink, synthetic

pytestmark = pytest.mark.gpu

N_DATES = (0, 1, 63, 64, 65, 257, 1421)
N_PIX = (0, 1, 3, 100)
COVERS = (('span', pu.SPAN), ('extend', pu.EXTEND))
DTYPES = (('float32', pu.F32), ('int16', pu.I16))


@pytest.fixture(scope='module')
def ctx():
    c = ccdgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def table100():
    return pu.random_table(21, 100)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _assert_exact(ctx, off, rows, dates, what, avg=365.2425):
    B = ctx.coefficient_matrix(dates, avg)
    for cname, cover in COVERS:
        idx = pu.select(off, rows, dates, cover)
        v = pu.evaluate(off, rows, idx, B)
        for dname, dtype in DTYPES:
            got, got_idx = ctx.predict(off, rows, dates, avg_days_yr=avg, cover=cname, dtype=dname)
            _same(got_idx, idx, (what, cname, dname, 'seg_index'))
            _same(got, pu.convert(v, idx, dtype), (what, cname, dname))
        again, none = ctx.predict(off, rows, dates, avg_days_yr=avg, cover=cover, dtype=np.int16, seg_index=False)
        assert none is None
        _same(again, pu.convert(v, idx, pu.I16), (what, cname, 'no seg_index'))


@pytest.mark.parametrize('n_pix', N_PIX)
def test_exact_against_the_restatement(ctx, n_pix):
    """Every date count around the wave and block sizes, every row count of predict_util.COUNTS
    (none, pyccd.default's row, below, at and above the kernel's model cache, 70), both covers,
    both output types and seg_index; dates shuffled and repeated, drawn from the rows' own edges."""
    off, rows = pu.random_table(20 + n_pix, n_pix)
    for n_dates in N_DATES:
        _assert_exact(ctx, off, rows, pu.sample_dates(n_dates, rows, n_dates), (n_pix, n_dates))


def test_every_edge_date(ctx, table100):
    """Every sday, eday, sday - 1 and eday + 1 of a 100-pixel table, shuffled, some twice; and a
    year of another length."""
    off, rows = table100
    edges = pu.edge_dates(rows)
    rng = np.random.default_rng(22)
    dates = rng.permutation(np.concatenate([edges, edges[::7]]))
    _assert_exact(ctx, off, rows, dates, 'edges')
    _assert_exact(ctx, off, rows, dates[:300], 'julian year', avg=365.25)
    idx = pu.select(off, rows, dates, pu.SPAN)
    assert idx.max() == 69 and (idx == -1).any() and (pu.select(off, rows, dates, pu.EXTEND) != idx).any()


def test_conversions(ctx):
    """Intercept-only models are exact: halves go to even, +-1e6 saturates; a NaN coefficient is
    NaN / -9999; a date no row holds is the fill, seg_index -1."""
    icpt = np.float32([0.5, 1.5, -0.5, 2.5, 1e6, -1e6, 7.0])
    rows = np.zeros(3, dtype=abi.ROW_DTYPE)
    rows['sday'], rows['eday'], rows['has_model'] = 730000, 730100, 1
    rows['intercept'][:] = icpt
    rows['coef'][1, :, 3] = np.nan
    rows['intercept'][2] = icpt[::-1]
    off = np.int64([0, 1, 2, 3])
    dates = np.int64([730000, 729999, 730100, 730101, 730050])
    inside = np.array([True, False, True, False, True])
    f32, idx = ctx.predict(off, rows, dates, dtype='float32')
    i16, idx2 = ctx.predict(off, rows, dates, dtype='int16')
    np.testing.assert_array_equal(idx, np.where(inside, 0, -1)[None].repeat(3, axis=0))
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(f32[:, 0, inside], icpt[:, None].repeat(3, axis=1))
    np.testing.assert_array_equal(i16[:, 0, inside], np.int16([0, 2, 0, 2, 32767, -32768, 7])[:, None].repeat(3, axis=1))
    np.testing.assert_array_equal(i16[:, 2, inside], np.int16([7, -32768, 32767, 2, 0, 2, 0])[:, None].repeat(3, axis=1))
    assert (f32[:, 1].view(np.uint32) == 0x7fc00000).all() and (i16[:, 1] == -9999).all()  # NaN coefficient
    assert (f32[:, :, ~inside].view(np.uint32) == 0x7fc00000).all() and (i16[:, :, ~inside] == -9999).all()
    # extend: the model holds after its end, not before its start
    i16e, idxe = ctx.predict(off, rows, dates, cover='extend', dtype='int16')
    np.testing.assert_array_equal(idxe[0], [0, -1, 0, 0, 0])
    np.testing.assert_array_equal(i16e[0, 0], [0, -9999, 0, 0, 0])


def test_basis(ctx):
    """The t column is the dates; cos / sin within 4 * 2^-52 of the reference's coefficient_matrix:
    OCML documents at most 2 ulp for double sin / cos, glibc at most 1, values in [-1, 1] have
    ulp <= 2^-52, the rest is margin (the arguments are the same lines, so bit-equal)."""
    rng = np.random.default_rng(23)
    dates = np.concatenate([[1, abi.PREDICT_MAX_DATE, 730000, 730000], rng.integers(1, abi.PREDICT_MAX_DATE + 1, 500),
                            rng.integers(723000, 740000, 917)]).astype(np.int64)
    for avg in (365.2425, 365.25):
        got = ctx.coefficient_matrix(dates, avg)
        ref = ccd_ref.coefficient_matrix(dates, avg, 8)
        assert got.shape == (dates.shape[0], 7) and got.dtype == np.float64
        np.testing.assert_array_equal(got[:, 0], dates)
        err = np.abs(got[:, 1:] - ref[:, 1:]).max()
        print('basis: max |device - reference| = %.3g (bound %.3g)' % (err, 4 * 2.0 ** -52))
        assert err <= 4 * 2.0 ** -52
    assert ctx.coefficient_matrix(np.zeros(0, np.int64)).shape == (0, 7)


def test_independent_of_the_device_basis(ctx, table100):
    """The values in double, before any narrowing to float32 -- the restatement fed the device's
    basis, which test_exact shows to be what the device evaluates -- against the restatement with
    numpy's own basis: within 2^-47 S, S = |intercept| + |c0 t| + sum |ck| (at most 15 roundings a
    side of at most 2^-53 S each, plus the basis term of at most 2^-50 S).  And the device's float32
    output itself against numpy's value: that bound plus float32's rounding, 2^-24 |v|.  No value is
    exempt."""
    off, rows = table100
    dates = pu.sample_dates(24, rows, 1421)
    idx = pu.select(off, rows, dates, pu.EXTEND)
    v_np = pu.evaluate(off, rows, idx, pu.basis(dates))
    v_dev = pu.evaluate(off, rows, idx, ctx.coefficient_matrix(dates))
    s = pu.scale(off, rows, idx, dates)
    taken = (idx >= 0)[None].repeat(7, axis=0)
    assert taken.sum() > 100000 and s[taken].min() > 0
    ratio = (np.abs(v_dev - v_np)[taken] / s[taken]).max()
    print('values: max |device basis - numpy basis| / S = %.3g (bound %.3g)' % (ratio, 2.0 ** -47))
    assert (np.abs(v_dev - v_np)[taken] <= 2.0 ** -47 * s[taken]).all()
    got, _ = ctx.predict(off, rows, dates, cover='extend', dtype='float32')
    assert not np.isnan(got[taken]).any() and np.isnan(got[~taken]).all()
    bound = 2.0 ** -47 * s[taken] + 2.0 ** -24 * np.abs(v_np[taken])
    assert (np.abs(got[taken].astype(np.float64) - v_np[taken]) <= bound).all()


def test_slab_independence(table100):
    """Contexts that keep 1 and 7 pixels on the device at a time give the bytes of the default."""
    off, rows = table100
    dates = pu.sample_dates(25, rows, 130)
    results = {}
    old = os.environ.get('CCDGPU_PREDICT_SLAB_PIXELS')
    try:
        for slab in (None, '1', '7'):
            os.environ.pop('CCDGPU_PREDICT_SLAB_PIXELS', None)
            if slab is not None:
                os.environ['CCDGPU_PREDICT_SLAB_PIXELS'] = slab
            c = ccdgpu.Context(0)
            try:
                results[slab] = [c.predict(off, rows, dates, cover=cover, dtype=dtype) for cover, _ in COVERS for dtype, _ in DTYPES]
            finally:
                c.close()
    finally:
        os.environ.pop('CCDGPU_PREDICT_SLAB_PIXELS', None)
        if old is not None:
            os.environ['CCDGPU_PREDICT_SLAB_PIXELS'] = old
    for slab in ('1', '7'):
        for (v, i), (v0, i0) in zip(results[slab], results[None]):
            _same(v, v0, slab)
            _same(i, i0, slab)
    assert not np.isnan(results[None][0][0]).all()
    idx = pu.select(off, rows, dates, pu.SPAN)
    _same(results[None][0][1], idx, 'default context')


def test_caller_buffers(ctx, table100):
    """out / seg_index arrays of the caller's (page-locked, reused) receive the same bytes."""
    off, rows = table100
    dates = pu.sample_dates(26, rows, 65)
    out = ccdgpu.pinned_empty((7, 100, 65), np.int16)
    idx = ccdgpu.pinned_empty((100, 65), np.int32)
    for cover, _ in COVERS:
        out[...], idx[...] = 1, 7
        want, wi = ctx.predict(off, rows, dates, cover=cover, dtype='int16')
        got, gi = ctx.predict(off, rows, dates, cover=cover, dtype='int16', out=out, seg_index=idx)
        assert got is out and gi is idx
        _same(np.asarray(out), want, cover)
        _same(np.asarray(idx), wi, cover)
    for bad in (np.empty((7, 100, 65), np.float32), np.empty((7, 100, 64), np.int16), out[:, :, ::-1]):
        with pytest.raises(ValueError, match='out must be'):
            ctx.predict(off, rows, dates, dtype='int16', out=bad)
    with pytest.raises(ValueError, match='seg_index must be'):
        ctx.predict(off, rows, dates, seg_index=np.empty((100, 65), np.int64))


def _chained_equals_table(ctx, batch, locs, what):
    """predict_rows of every chip at its own dates and at 33 annual dates against predict on the
    chip's fetched rows; returns chip 0's fetched rows and int16 / float32 results for the caller."""
    kept = None
    for c, (cx, cy) in enumerate(locs):
        off, rows, mask = ctx.fetch_rows(c, cx, cy)
        own = batch.chip(c)[0]
        assert rows.shape[0] > off.shape[0] - 1  # more than one segment somewhere
        if c == 0:
            kept = (off, rows, mask, own)
        for dates in (own, synthetic.annual_dates(1985, 2017)):
            for cname, _ in COVERS:
                for dname, _ in DTYPES:
                    got, gi = ctx.predict_rows(c, dates, cover=cname, dtype=dname)
                    want, wi = ctx.predict(off, rows, dates, cover=cname, dtype=dname)
                    assert got.shape == (7, int(batch.n_pix[c]), len(dates))
                    _same(got, want, (what, c, cname, dname))
                    _same(gi, wi, (what, c, cname, dname, 'seg_index'))
        assert (gi >= 0).any()
    return kept


def test_chained_equals_table(ctx):
    """64 pixels of a C5 chip and 64 of a C3 chip in one batch: the chained path (the run's segments
    on the device) gives the bytes of the table path on the fetched rows -- after a plain run, after
    a run_slot_begin_rows / run_slot_end_rows run, and through ccdc.synthetic.predict on the sink's
    segment table."""
    chips = [synth.chip(synth.config(5), 2, 0, 64), synth.chip(synth.config(3), 1, 64, 64)]
    locs = [(-585, 2805), (2415, 2805)]
    batch = ctx.stage_chips(chips)
    ctx.run()
    off, rows, mask, own = _chained_equals_table(ctx, batch, locs, 'run')
    # through the Arrow segment table of the sink
    tabs = sink.tables(locs[0][0], locs[0][1], own, off, rows, mask)
    for cname, _ in COVERS:
        for dname, _ in DTYPES:
            keys, values, idx = synthetic.predict(tabs['segment'], own, cover=cname, dtype=dname, context=ctx)
            want, wi = ctx.predict_rows(0, own, cover=cname, dtype=dname)
            np.testing.assert_array_equal(keys[:, 2:], rows[['px', 'py']][off[:-1]].tolist())
            _same(values, want, ('table', cname, dname))
            _same(idx, wi, ('table', cname, dname))
    # observations minus the model at the chip's own dates: the layout of spectra
    resid = batch.chip(0)[1] - ctx.predict_rows(0, own)[0]
    assert resid.shape == batch.chip(0)[1].shape
    buf = np.zeros((7, 64, len(own)), np.float32)
    got, none = ctx.predict_rows(0, own, out=buf, seg_index=False)
    assert got is buf and none is None
    _same(buf, ctx.predict_rows(0, own)[0], 'caller buffer')
    # the batch chain
    bufs = ccdgpu.RowsBuffers(pinned=True)
    cx, cy = [l[0] for l in locs], [l[1] for l in locs]
    ctx.stage_slot_chips(0, batch)
    ctx.run_slot_begin_rows(0, cx, cy, bufs)
    boff, brows, _ = ctx.run_slot_end_rows()
    assert brows.shape[0] == boff[-1]
    _chained_equals_table(ctx, batch, locs, 'rows chain')


def test_predict_chips_equals_the_tables(ctx):
    """ccdc.synthetic.predict_chips (chipmunk chips in, detection, prediction behind it) against
    synthetic.predict over the segment tables pyccd.detect_chips_tables gives for the same chips:
    at each chip's own dates (input order) and at dates of the caller's."""
    from ccdc import chipmunk, pyccd
    locs = [(-585, 2805), (2415, 2805)]
    chips, own = [], {}
    for i, (cx, cy) in enumerate(locs):
        d, s, q = synth.chip(synth.config(5), 4, 100 * i, 100)
        order = np.argsort(d)[::-1]
        own[cx, cy] = d[order]
        chips += chipmunk.chip_response(cx, cy, d[order], s[:, :, order].copy(), q[:, order].copy())
    tables = dict(pyccd.detect_chips_tables(chips, context=ctx))
    annual = [date.fromordinal(int(o)).isoformat() for o in synthetic.annual_dates(1990, 2010)]
    for dates_of, kw in ((None, {}), (lambda cx, cy, dates: annual, {'cover': 'extend', 'dtype': 'int16'})):
        got = synthetic.predict_chips(chips, dates_of=dates_of, context=ctx, **kw)
        assert [k for k, _, _, _ in got] == locs
        for (cx, cy), at, values, idx in got:
            np.testing.assert_array_equal(at, own[cx, cy] if dates_of is None else synthetic.ordinals(annual))
            keys, want, wi = synthetic.predict(tables[cx, cy]['segment'], at, context=ctx, **kw)
            assert keys.shape == (100, 4) and (keys[:, 0] == cx).all()
            _same(values, want, (cx, cy, kw))
            _same(idx, wi, (cx, cy, kw))
            assert (idx >= 0).any()


def _raw_predict_rows(c, chip, dates, out, idx):
    secs = ctypes.c_double(0.0)
    return ccdgpu.lib().ccdgpu_predict_rows(c._ctx, chip, dates.shape[0], dates.ctypes.data, 365.2425, 0, 0, out.ctypes.data,
                                            idx.ctypes.data, ctypes.byref(secs))


def test_errors_write_nothing():
    c = ccdgpu.Context(0)
    try:
        dates = synthetic.annual_dates(1990, 1999)
        out = np.full((7, 64, 10), 123.0, dtype=np.float32)
        idx = np.full((64, 10), 77, dtype=np.int32)

        def refused(chip, match):
            assert _raw_predict_rows(c, chip, dates, out, idx) == abi.E_INVAL
            assert match in ccdgpu.last_error(), ccdgpu.last_error()
            assert (out == 123.0).all() and (idx == 77).all()

        refused(0, 'no completed run')
        with pytest.raises(ccdgpu.CcdGpuError) as e:
            c.predict_rows(0, dates)
        assert e.value.code == abi.E_INVAL
        batch = ccdgpu.ChipBatch.from_chips([synth.chip(synth.config(3), 0, 0, 64)], pinned=True)
        c.stage_chips(batch)
        refused(0, 'no completed run')  # staged, not run
        c.run()
        refused(1, 'chip 1 is outside')
        refused(-1, 'chip -1 is outside')
        with pytest.raises(ccdgpu.CcdGpuError) as e:
            c.predict_rows(1, dates)
        assert e.value.code == abi.E_INVAL
        bad = dates.copy()
        bad[3] = 0
        assert _raw_predict_rows(c, 0, bad, out, idx) == abi.E_INVAL and 'dates[3]' in ccdgpu.last_error()
        assert (out == 123.0).all() and (idx == 77).all()
        good, _ = c.predict_rows(0, dates)
        off, rows = pu.random_table(31, 5)
        c.stage_slot_chips(0, batch)
        c.run_slot_begin(0)
        try:
            refused(0, 'not finished')
            for call in (lambda: c.predict(off, rows, dates), lambda: c.predict_rows(0, dates),
                         lambda: c.coefficient_matrix(dates)):
                with pytest.raises(ccdgpu.CcdGpuError) as e:
                    call()
                assert e.value.code == abi.E_INVAL and 'not finished' in e.value.message
        finally:
            c.run_slot_end()
        _same(c.predict_rows(0, dates)[0], good, 'after the pending run')
        with pytest.raises(ccdgpu.CcdGpuError) as e:  # the table path runs the check first
            c.predict(off, rows, bad)
        assert e.value.code == abi.E_INVAL and 'dates[3]' in e.value.message
        with pytest.raises(ValueError):
            c.predict(off, rows, dates, cover='nearest')
        # a detect_batch of another size is the last run from then on: the output is sized by it
        d, s, q = synth.chip(synth.config(3), 1, 0, 100)
        c.detect_batch(d, s, q)
        got, gi = c.predict_rows(0, dates)
        assert got.shape == (7, 100, 10) and gi.shape == (100, 10)
        roff, rrows, _ = c.fetch_rows(0, 0, 0)
        _same(got, c.predict(roff, rrows, dates)[0], 'after detect_batch')
    finally:
        c.close()
