"""Annual change and land-cover product rasters, host side: the numpy restatement of the rule
(tests/products_util.py) against itself and its coverage of the rule's branches, the library's year
window and request check (no device needed), the stand-alone sanitizer program of the checks, and the
table handling of ccdc.products with the device call stubbed.  The device comparisons are in
tests/test_gpu_products.py."""
import ctypes
import os
import re
import subprocess
from datetime import date

import numpy as np
import pytest

import ccdgpu
import predict_util as pu
import products_util as qu
from ccdgpu import abi
from ccdc import products, sink

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _par(n_classes, cover, **kw):
    return qu.params(n_classes=n_classes, cover=cover, **kw)


def test_abi_mirrors_the_header():
    text = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    body = text[text.index('struct ccdgpu_products {'):]
    body = body[:body.index('};')]
    assert re.findall(r'\*(\w+)', body) == [n for n, _ in abi.PRODUCTS] == list(qu.NAMES)
    assert ctypes.sizeof(abi.Products) == 10 * ctypes.sizeof(ctypes.c_void_p)
    body = text[text.index('typedef struct ccdgpu_product_params'):text.index('} ccdgpu_product_params;')]
    assert re.findall(r'\b(\w+)(?:\[32\])?;', re.sub(r'/\*.*?\*/', '', body)) ==[n for n, _ in abi.ProductParams._fields_]
    assert ctypes.sizeof(abi.ProductParams) == 56
    p, q = ccdgpu.product_params(), abi.default_product_params()
    assert (p.bot, p.mag_bands, p.cover, p.n_classes) == (q.bot, q.mag_bands, q.cover, q.n_classes)
    assert (p.bot, p.mag_bands, p.cover, p.n_classes) == (date(1982, 1, 1).toordinal(), 0x3E, abi.COVER_EXTEND, 0)
    assert list(p.labels) == list(q.labels) == list(range(1, 33))
    for name in ('ccdgpu_product_params_default', 'ccdgpu_year_window', 'ccdgpu_products_check', 'ccdgpu_products',
                 'ccdgpu_products_rows', 'ccdgpu_chip_row_count'):
        assert name in ccdgpu.EXPORTS and hasattr(ccdgpu.lib(), name)
    dev = open(os.path.join(ROOT, 'lcmap-firebird_amd', 'csrc', 'ccd_products.h')).read()
    assert 'uint32_t pad[2];' in dev  # (the 32-byte record the kernels share)


def test_loop_and_vectorised_restatements_agree():
    """Every product of the generated tables, one value at a time and vectorised: the same bytes."""
    for seed, n_pix, n_dates, nc, cover in qu.grid():
        if n_pix > 65 and n_dates > 2:
            n_pix = 66  # (the loop is slow; 66 pixels hold every row count 11 times)
        off, rows, dates, raw = qu.case(seed, n_pix, n_dates, nc)
        par = _par(nc, cover)
        a, b = qu.products(off, rows, dates, raw, par), qu.products_loop(off, rows, dates, raw, par)
        assert set(a) == set(b) == set(qu.NAMES)
        for name in qu.NAMES:
            assert a[name].dtype == b[name].dtype == np.dtype(abi.PRODUCT_DTYPES[name])
            assert a[name].shape == b[name].shape == (n_dates, n_pix)
            assert a[name].tobytes() == b[name].tobytes(), (name, seed, n_pix, n_dates, nc, cover)
        change = qu.products(off, rows, dates, None, par)
        assert set(change) == set(abi.CHANGE_PRODUCTS)
        for name in abi.CHANGE_PRODUCTS:
            assert change[name].tobytes() == a[name].tobytes()
    # other parameters: another beginning of time, one magnitude band, labels of the caller's
    off, rows, dates, raw = qu.case(7, 40, 33, 9)
    par = _par(9, abi.COVER_SPAN, bot=date(1995, 1, 1).toordinal(), mag_bands=0x08, labels=np.arange(250, 218, -1))
    a, b = qu.products(off, rows, dates, raw, par), qu.products_loop(off, rows, dates, raw, par)
    for name in qu.NAMES:
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a['lcpri'].max() > 200 and np.isnan(a['scmag']).any()


def test_generated_tables_reach_every_branch():
    """A coverage condition on the reference alone, so no product test is vacuous."""
    seen = {n: set() for n in qu.NAMES}
    bot_branch = before_bot = False
    for seed, n_pix, n_dates, nc, cover in qu.grid():
        off, rows, dates, raw = qu.case(seed, n_pix, n_dates, nc)
        got = qu.products(off, rows, dates, raw, _par(nc, cover))
        for n in qu.NAMES:
            v = got[n]
            seen[n].update(np.unique(v[~np.isnan(v)] if v.dtype.kind == 'f' else v).tolist())
        if n_pix and n_dates:
            empty = np.flatnonzero(np.diff(off) == 0)
            t = np.asarray(dates)
            if empty.size:
                late = t >= abi.PRODUCT_BOT
                bot_branch |= bool((got['scstab'][late][:, empty] == np.minimum(t[late] - abi.PRODUCT_BOT, 65535)[:, None]).all()
                                   and late.any() and (got['scstab'][late][:, empty] > 0).any())
                before_bot |= bool((~late).any() and (got['scstab'][~late][:, empty] == 0).all())
    for n in qu.NAMES:
        assert 0 in seen[n] and len(seen[n]) > 1, n
    assert 1 in seen['sctime'] and (365 in seen['sctime'] or 366 in seen['sctime'])
    assert bot_branch and before_bot
    assert max(seen['scmqa']) == 255
    assert max(seen['lcpconf']) == 100 and any(0 < v < 100 for v in seen['lcpconf'])
    assert any(v for v in seen['lcachg'])
    # the clamp at 65535 days: a break long before the date
    off, rows = pu.random_table(1, 1, counts=(1,))
    rows['chprob'], rows['bday'], rows['sday'], rows['eday'] = 1.0, 5, 2, 4
    got = qu.products(off, rows, [date(1990, 7, 1).toordinal()])
    assert got['sclast'][0, 0] == got['scstab'][0, 0] == 65535


def test_year_window_against_datetime():
    rng = np.random.default_rng(5)
    special = [1, 365, 366, 367, date.max.toordinal(), date.max.toordinal() - 364, date.max.toordinal() - 365]
    for y in (1600, 1900, 1999, 2000, 2001, 2004, 2100, 2400):
        special += [date(y, 1, 1).toordinal(), date(y, 12, 31).toordinal(), date(y, 2, 28).toordinal() + 1, date(y, 7, 1).toordinal()]
    t = np.concatenate([rng.integers(1, date.max.toordinal() + 1, 10000), special]).astype(np.int64)
    a, b = ccdgpu.year_window(t)
    wa, wb = qu.year_window(t)
    np.testing.assert_array_equal(a, wa)
    np.testing.assert_array_equal(b, wb)
    assert ((a <= t) & (t < b)).all() and set((b - a).tolist()) == {365, 366}
    for bad in (0, -5, date.max.toordinal() + 1):
        with pytest.raises(ValueError, match='outside 1'):
            ccdgpu.year_window([bad])


def test_products_check_names_each_malformed_input():
    off, rows, dates, raw = qu.case(3, 9, 2, 4)
    cover_par = lambda **kw: ccdgpu.product_params(n_classes=4, **kw)  # noqa: E731
    # accepted
    ccdgpu.products_check(off, rows, dates)
    ccdgpu.products_check(off, rows, dates, rfrawp=raw, params=cover_par(), want=abi.COVER_PRODUCTS)
    ccdgpu.products_check(off, rows, dates, rfrawp=raw, params=cover_par(cover='span'), want=('lcachg',))
    ccdgpu.products_check([0], None, [], n_pix=0)  # nothing at all is fine
    ccdgpu.products_check(off, rows, [1, abi.PREDICT_MAX_DATE])
    ccdgpu.products_check(off, rows, dates, params=ccdgpu.product_params(bot=1, mag_bands=0, n_classes=32))
    ccdgpu.products_check(off, rows, dates, params=ccdgpu.product_params(bot=abi.PREDICT_MAX_DATE, mag_bands=0x7F))
    zero_past = ccdgpu.product_params(labels=[1, 2, 3, 4, 0], n_classes=4)
    ccdgpu.products_check(off, rows, dates, rfrawp=raw, params=zero_past, want=('lcpri',))

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ccdgpu.products_check(*args, **kw)

    # what ccdgpu_predict_check refuses, by the product check's own name
    refused(r'products: n_pix must be >= 0', off, rows, dates, n_pix=-1)
    refused(r'products: n_rows must be >= 0', off, rows, dates, n_rows=-1)
    refused(r'products: row_offsets is NULL', None, rows, dates, n_pix=1)
    refused(r'products: rows is NULL', off, None, dates, n_rows=int(off[-1]))
    refused(r'products: row_offsets\[0\] must be 0', off + 1, rows, dates, n_rows=int(off[-1]) + 1)
    down = off.copy()
    down[4] = down[3] - 1
    refused(r'products: row_offsets decrease at pixel 3', down, rows, dates)
    refused(r'products: row_offsets\[n_pix\] is', off, rows[:-1], dates)
    refused(r'products: dates is NULL', off, rows, None)
    refused(r'products: dates\[1\] = 0 is outside', off, rows, [5, 0])
    refused(r'products: dates\[0\] = %d is outside' % (abi.PREDICT_MAX_DATE + 1), off, rows, [abi.PREDICT_MAX_DATE + 1])
    lib = ccdgpu.lib()
    p, o = ccdgpu.product_params(), abi.Products()
    o.sctime = 1
    o8 = np.ascontiguousarray(off, dtype=np.int64)
    assert lib.ccdgpu_products_check(0, o8.ctypes.data, 0, None, None, -1, None, ctypes.byref(p), ctypes.byref(o)) == abi.E_INVAL
    assert 'n_dates must be >= 0' in ccdgpu.last_error()
    assert lib.ccdgpu_products_check(0, o8.ctypes.data, 0, None, None, 2 ** 31, o8.ctypes.data, ctypes.byref(p),
                                     ctypes.byref(o)) == abi.E_INVAL
    assert 'n_dates must be < 2^31' in ccdgpu.last_error()
    # the product request's own
    refused(r'products: params is NULL', off, rows, dates, params=False)
    assert lib.ccdgpu_products_check(0, o8.ctypes.data, 0, None, None, 0, None, ctypes.byref(p), None) == abi.E_INVAL
    assert 'out is NULL' in ccdgpu.last_error()
    for bot in (0, -1, abi.PREDICT_MAX_DATE + 1):
        refused(r'products: bot = %d is outside' % bot, off, rows, dates, params=ccdgpu.product_params(bot=bot))
    refused(r'mag_bands must only use bits 0..6', off, rows, dates, params=ccdgpu.product_params(mag_bands=0x80))
    for nc in (-1, 33):
        refused(r'n_classes must be in \[0, 32\], got %d' % nc, off, rows, dates, params=ccdgpu.product_params(n_classes=nc))
    refused(r'labels\[2\] is 0', off, rows, dates, params=ccdgpu.product_params(labels=[5, 6, 0, 7]))
    refused(r'unknown cover 2', off, rows, dates, params=ccdgpu.product_params(cover=2))
    for name in abi.COVER_PRODUCTS:
        refused(r'cover product is requested but rfrawp is NULL', off, rows, dates, params=cover_par(), want=(name,))
        refused(r'cover product is requested but n_classes is 0', off, rows, dates, rfrawp=raw, want=('sctime', name))
    refused(r'no product is requested', off, rows, dates, want=())
    refused(r'no product is requested', off, rows, dates, rfrawp=raw, params=cover_par(), want=())


def test_native_product_checks_under_sanitizers(tmp_path):
    """tests/native/product_checks.cpp: ccdgpu_products_check and ccdgpu_year_window
    (csrc/ccdgpu_checks.cpp, no HIP in it) in a stand-alone program built with
    -fsanitize=address,undefined -- every argument in a heap block of exactly its size."""
    csrc = os.path.join(ROOT, 'lcmap-firebird_amd', 'csrc')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    probe = subprocess.run(['gcc', '-fsanitize=address,undefined', '-x', 'c', '-o', str(tmp_path / 'probe'), '-'],
                           input='int main(void){return 0;}', capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip('the compiler cannot link -fsanitize=address,undefined')
    exe = str(tmp_path / 'product_checks')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17'] + san + ['-I', os.path.join(ROOT, 'include'), '-o', exe,
                                                               os.path.join(HERE, 'native', 'product_checks.cpp'),
                                                               os.path.join(csrc, 'ccdgpu_checks.cpp')], check=True)
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith('ok'), out.stdout


class _StubContext(object):
    """Context.products by the restatement, recording what it was given."""

    def products(self, row_offsets, rows, dates, rfrawp=None, labels=None, cover='extend', bot=None, mag_bands=None, want=None):
        self.given = (row_offsets, rows, dates, rfrawp)
        nc = 0 if rfrawp is None else rfrawp.shape[1]
        par = qu.params(n_classes=nc, cover=abi.COVERS[cover], labels=labels, **({} if bot is None else {'bot': bot}))
        got = qu.products(row_offsets, rows, dates, rfrawp, par)
        return got if want is None else {n: got[n] for n in want}


def test_annual_and_rasters_handle_the_table():
    """ccdc.products.annual over the sink's segment table: keys and rows as synthetic.rows_from_table
    gives them, the table's rfrawp column (or a matrix of the caller's) permuted with the rows, null
    predictions NaN; rasters scatters a plane by px / py."""
    cx, cy = -585, 2805
    off, rows = qu.table(11, 6, qu.product_dates(33))
    rows['px'] = cx + 30 * np.repeat([0, 1, 2, 99, 0, 99], np.diff(off))
    rows['py'] = cy - 30 * np.repeat([0, 0, 0, 0, 1, 99], np.diff(off))
    raw = qu.rfrawp_for(11, rows, 9)
    dates = qu.product_dates(33)
    stub = _StubContext()
    # pixel 0 has no rows and so does not appear in the table; 5 pixels do
    table = sink.segment_table(cx, cy, rows, raw)
    keys, got = products.annual(table, dates, context=stub, cover='span')
    assert keys.shape == (5, 4) and set(got) == set(qu.NAMES)
    np.testing.assert_array_equal(stub.given[0], off[1:] - off[1])
    assert stub.given[1].tobytes() == rows.tobytes()
    null = np.isnan(raw).any(axis=1)
    np.testing.assert_array_equal(np.isnan(stub.given[3]).all(axis=1), null)
    assert stub.given[3][~null].tobytes() == raw[~null].tobytes()
    want = qu.products(off[1:], rows, dates, np.where(null[:, None], np.nan, raw).astype(np.float32), qu.params(n_classes=9, cover=abi.COVER_SPAN))
    for n in qu.NAMES:
        assert got[n].tobytes() == want[n].tobytes(), n
    # the table's rows in another order: pixels in first-appearance order, rfrawp with its rows
    perm = np.random.default_rng(2).permutation(rows.shape[0])
    keys2, got2 = products.annual(table.take(perm), dates, context=stub, cover='span')
    back = [keys2[:, 2:].tolist().index(k) for k in keys[:, 2:].tolist()]
    pix = np.repeat(np.arange(5), np.diff(off[1:]))
    stable = all((np.diff(perm.argsort()[pix == p]) > 0).all() for p in range(5))
    if stable:  # (a pixel's rows kept their table order: every product is the same)
        for n in qu.NAMES:
            np.testing.assert_array_equal(got2[n][:, back], got[n])
    np.testing.assert_array_equal(got2['sclast'][:, back], got['sclast'])  # (does not depend on the order of a pixel's rows)
    # a matrix of the caller's; no predictions at all
    keys3, got3 = products.annual(sink.segment_table(cx, cy, rows), dates, rfrawp=raw, context=stub, cover='span', want=('lcpri', 'lcachg'))
    assert set(got3) == {'lcpri', 'lcachg'} and got3['lcpri'].tobytes() == got['lcpri'].tobytes()
    keys4, got4 = products.annual(sink.segment_table(cx, cy, rows), dates, context=stub)
    assert set(got4) == set(abi.CHANGE_PRODUCTS) and stub.given[3] is None
    with pytest.raises(ValueError, match='rfrawp must be'):
        products.annual(table, dates, rfrawp=raw[:-1], context=stub)
    # rasters
    r = products.rasters(keys, got['scstab'][3])
    assert list(r) == [(cx, cy)] and r[cx, cy].shape == (100, 100) and r[cx, cy].dtype == np.uint16
    plane = got['scstab'][3]
    assert r[cx, cy][0, 1] == plane[0] and r[cx, cy][0, 2] == plane[1] and r[cx, cy][0, 99] == plane[2]
    assert r[cx, cy][1, 0] == plane[3] and r[cx, cy][99, 99] == plane[4]
    assert np.count_nonzero(r[cx, cy]) <= 5
    two = np.concatenate([keys, keys + [3000, 0, 3000, 0]])
    r2 = products.rasters(two, np.concatenate([plane, plane + 1]), width=100)
    assert list(r2) == [(cx, cy), (cx + 3000, cy)] and r2[cx + 3000, cy][99, 99] == plane[4] + 1
    with pytest.raises(ValueError, match='outside'):
        products.rasters(keys, plane, width=50)
    with pytest.raises(ValueError, match='pixels'):
        products.rasters(keys, plane[:-1])
