"""Prediction of band values from segment models, host side: the Arrow table -> rows conversion of
ccdc.synthetic, the argument check of the library (ccdgpu_predict_check needs no device), and the
numpy restatement of the rule (tests/predict_util.py) against itself and against the oracle's
predict.  The device comparisons are in tests/test_gpu_synthetic.py."""
import os
import re
from datetime import date
from types import SimpleNamespace

import numpy as np
import pytest

import ccd_ref
import ccdgpu
import predict_util as pu
from ccdgpu import abi
from ccdc import sink, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_mirrors_the_headers():
    text = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    for name, value in (('CCDGPU_COVER_SPAN', abi.COVER_SPAN), ('CCDGPU_COVER_EXTEND', abi.COVER_EXTEND),
                        ('CCDGPU_PREDICT_F32', abi.PREDICT_F32), ('CCDGPU_PREDICT_I16', abi.PREDICT_I16)):
        assert re.search(r'\b%s = %d\b' % (name, value), text), name
    assert int(re.search(r'#define CCDGPU_PREDICT_MAX_DATE (\d+)', text).group(1)) == abi.PREDICT_MAX_DATE == date.max.toordinal()
    kernel_h = open(os.path.join(ROOT, 'lcmap-firebird_amd', 'csrc', 'ccd_predict.h')).read()
    assert int(re.search(r'#define CCD_PREDICT_CACHE_ROWS (\d+)', kernel_h).group(1)) == abi.PREDICT_CACHE_ROWS
    assert abi.PREDICT_CACHE_ROWS + 1 in pu.COUNTS and 70 in pu.COUNTS and 0 in pu.COUNTS and 'd' in pu.COUNTS


def _hand_rows():
    """Three pixels: two models, pyccd.default's row, one model without a break day."""
    off, rows = pu.random_table(3, 3, counts=(2, 'd', 1))
    rows['px'], rows['py'] = [100, 100, 130, 160], [200, 200, 200, 170]
    rows['bday'][3] = 0
    return off, rows


def test_rows_from_table_round_trips_the_sink():
    off, rows = _hand_rows()
    table = sink.segment_table(-585, 2805, rows)
    assert table['chprob'].null_count == 1 and table['bday'].null_count == 1
    keys, off2, rows2 = synthetic.rows_from_table(table)
    np.testing.assert_array_equal(keys, [[-585, 2805, 100, 200], [-585, 2805, 130, 200], [-585, 2805, 160, 170]])
    np.testing.assert_array_equal(off2, off)
    assert rows2.dtype == abi.ROW_DTYPE and rows2.tobytes() == rows.tobytes()
    # a pixel's rows apart in the table: together again, pixels in first-appearance order
    mixed = table.take([3, 0, 2, 1])
    keys, off3, rows3 = synthetic.rows_from_table(mixed)
    np.testing.assert_array_equal(keys[:, 2], [160, 100, 130])
    np.testing.assert_array_equal(off3, [0, 1, 3, 4])
    assert rows3.tobytes() == rows[[3, 0, 1, 2]].tobytes()
    keys, off0, rows0 = synthetic.rows_from_table(table.slice(0, 0))
    assert keys.shape == (0, 4) and off0.tolist() == [0] and rows0.shape == (0,)


def test_annual_dates_and_ordinals():
    got = synthetic.annual_dates(1985, 2017)
    assert got.dtype == np.int64 and got.shape == (33,)
    assert got[0] == date(1985, 7, 1).toordinal() and got[-1] == date(2017, 7, 1).toordinal()
    assert [date.fromordinal(int(o)).isoformat()[4:] for o in got] == ['-07-01'] * 33
    np.testing.assert_array_equal(synthetic.annual_dates(2000, 2001, month=2, day=29 - 1),
                                  [date(2000, 2, 28).toordinal(), date(2001, 2, 28).toordinal()])
    want = [date(1999, 12, 31).toordinal(), 1, date.max.toordinal()]
    for form in (want, np.int32(want), [date.fromordinal(o) for o in want], ['1999-12-31', '0001-01-01', '9999-12-31']):
        got = synthetic.ordinals(form)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, want)
    assert synthetic.ordinals([]).shape == (0,)


def test_predict_check_names_each_malformed_input():
    off, rows = pu.random_table(5, 9)
    dates = pu.sample_dates(5, rows, 40)
    ccdgpu.predict_check(off, rows, dates)
    ccdgpu.predict_check(off, rows, dates, 365.25, abi.COVER_EXTEND, abi.PREDICT_I16)
    ccdgpu.predict_check([0], None, [], n_pix=0)  # nothing at all is fine

    def rejected(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ccdgpu.predict_check(*args, **kw)

    rejected('row_offsets is NULL', None, rows, dates, n_pix=9)
    rejected('rows is NULL', off, None, dates, n_rows=rows.shape[0])
    rejected('dates is NULL', off, rows, None)
    bad = off.copy()
    bad[0] = 1
    rejected(r'row_offsets\[0\] must be 0', bad, rows, dates)
    bad = off.copy()
    bad[4] = bad[3] - 1
    rejected('row_offsets decrease at pixel 3', bad, rows, dates)
    rejected(r'row_offsets\[n_pix\] is %d, n_rows is %d' % (off[-1], off[-1] - 1), off, rows[:-1], dates)
    rejected('n_pix must be >= 0', off, rows, dates, n_pix=-1)
    rejected('n_rows must be >= 0', off, rows, dates, n_rows=-1)
    for i, v in ((0, 0), (7, -5), (39, abi.PREDICT_MAX_DATE + 1)):
        bad = dates.copy()
        bad[i] = v
        rejected(r'dates\[%d\] = %d is outside' % (i, v), off, rows, bad)
    ok = dates.copy()
    ok[0], ok[1] = 1, abi.PREDICT_MAX_DATE
    ccdgpu.predict_check(off, rows, ok)
    for avg in (0.0, -365.25, float('nan'), float('inf'), float('-inf')):
        rejected('avg_days_yr must be finite and > 0', off, rows, dates, avg)
    rejected('unknown cover 2', off, rows, dates, 365.2425, 2)
    rejected('unknown cover -1', off, rows, dates, 365.2425, -1)
    rejected('unknown dtype 2', off, rows, dates, 365.2425, 0, 2)
    lib = ccdgpu.lib()
    assert lib.ccdgpu_predict_check(0, off.ctypes.data, 0, None, -1, None, 365.2425, 0, 0) == abi.E_INVAL
    assert 'n_dates must be >= 0' in ccdgpu.last_error()


@pytest.mark.parametrize('cover', [pu.SPAN, pu.EXTEND])
def test_vectorised_selection_equals_the_loop(cover):
    off, rows = pu.random_table(7, 2 * len(pu.COUNTS))
    dates = np.concatenate([pu.edge_dates(rows), pu.sample_dates(7, rows, 50)])
    got = pu.select(off, rows, dates, cover)
    np.testing.assert_array_equal(got, pu.select_loop(off, rows, dates, cover))
    kind = np.arange(len(off) - 1) % len(pu.COUNTS)  # pixels without rows, and with pyccd.default's row only
    assert (got[kind == 0] == -1).all() and (got[kind == 1] == -1).all()
    assert (got >= 0).any() and (got == -1).any() and got.max() >= 64
    if cover == pu.EXTEND:  # extend takes at least what span takes
        span = pu.select(off, rows, dates, pu.SPAN)
        assert ((got >= 0) | (span < 0)).all() and ((got >= 0) & (span < 0)).any()


def test_conversions_of_the_restatement():
    v = np.array([0.5, 1.5, -0.5, 2.5, -1.5, 1e6, -1e6, np.nan, 32767.5, -32768.5, 7.0]).reshape(1, 1, -1).repeat(7, axis=0)
    idx = np.zeros((1, v.shape[2]), dtype=np.int32)
    idx[0, -1] = -1
    i16 = pu.convert(v, idx, pu.I16)[0, 0]
    np.testing.assert_array_equal(i16, [0, 2, 0, 2, -2, 32767, -32768, -9999, 32767, -32768, -9999])
    f32 = pu.convert(v, idx, pu.F32)[0, 0]
    assert f32.dtype == np.float32 and f32[:7].tolist() == [0.5, 1.5, -0.5, 2.5, -1.5, 1e6, -1e6]
    assert f32[[7, 10]].view(np.uint32).tolist() == [0x7fc00000] * 2


def test_restatement_against_the_oracle_on_single_models():
    """The oracle evaluates X @ coef + intercept (a dot product in BLAS's order, the intercept
    last); the restatement sums left to right from the intercept.  Each side makes at most 15
    roundings of at most 2^-53 S each, S = |intercept| + |c0 t| + sum |ck|; the bases are the same
    numpy lines.  So they agree within 2^-47 S, and no value is exempt."""
    off, rows = pu.random_table(11, 12, counts=(1,))
    dates = np.sort(pu.sample_dates(11, rows, 300))
    B = pu.basis(dates)
    np.testing.assert_array_equal(B, ccd_ref.coefficient_matrix(dates, 365.2425, 8))
    idx = np.zeros((12, 300), dtype=np.int32)  # every date takes the pixel's one model
    v = pu.evaluate(off, rows, idx, B)
    s = pu.scale(off, rows, idx, dates)
    p = SimpleNamespace(AVG_DAYS_YR=365.2425)
    for px in range(12):
        for b in range(7):
            model = SimpleNamespace(coef=rows['coef'][px, b].astype(np.float64), intercept=float(rows['intercept'][px, b]))
            ref = ccd_ref.predict(model, dates, p)
            assert (np.abs(v[b, px] - ref) <= 2.0 ** -47 * s[b, px]).all(), (px, b)
    assert s.min() > 0
