"""Annual change and land-cover product rasters on the HIP path (ccd_products.hip through
ccdgpu.Context.products / products_rows) against the numpy restatement of tests/products_util.py.
The rule fixes every comparison and the order and rounding of every operation, so all comparisons
are exact (bytes)."""
import os
from datetime import date

import numpy as np
import pytest

import ccdgpu
import forest_util
import products_util as qu
from ccdgpu import abi, synth
from ccdc import products, synthetic
from ccdc.randomforest import Forest

pytestmark = pytest.mark.gpu

COVERS = (('span', abi.COVER_SPAN), ('extend', abi.COVER_EXTEND))


@pytest.fixture(scope='module')
def ctx():
    c = ccdgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def case100():
    """100 pixels at 33 dates with 9 classes, and the restatement's products under both covers."""
    off, rows, dates, raw = qu.case(51, 100, 33, 9)
    want = {cover: qu.products(off, rows, dates, raw, qu.params(n_classes=9, cover=cover)) for _, cover in COVERS}
    return off, rows, dates, raw, want


def _same(got, want, what):
    assert set(got) == set(want), what
    for n in want:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (what, n)
        assert got[n].tobytes() == want[n].tobytes(), (what, n)


@pytest.mark.parametrize('n_pix', qu.N_PIX)
def test_exact_against_the_restatement(ctx, n_pix):
    """Every pixel count around the wave size and every date count, the class counts and covers going
    round (products_util.grid): all ten products, and the change products without an rfrawp."""
    for seed, np_, n_dates, nc, cover in qu.grid():
        if np_ != n_pix:
            continue
        off, rows, dates, raw = qu.case(seed, n_pix, n_dates, nc)
        want = qu.products(off, rows, dates, raw, qu.params(n_classes=nc, cover=cover))
        _same(ctx.products(off, rows, dates, rfrawp=raw, cover=cover), want, (seed, n_pix, n_dates, nc, cover))
        _same(ctx.products(off, rows, dates, cover=cover), {n: want[n] for n in abi.CHANGE_PRODUCTS}, (seed, 'change only'))


@pytest.mark.parametrize('nc', qu.N_CLASSES)
def test_every_class_count_under_both_covers(ctx, nc):
    off, rows, dates, raw = qu.case(60 + nc, 65, 33, nc)
    labels = np.arange(255, 223, -1)
    for cname, cover in COVERS:
        want = qu.products(off, rows, dates, raw, qu.params(n_classes=nc, cover=cover))
        _same(ctx.products(off, rows, dates, rfrawp=raw, cover=cname), want, (nc, cname))
        par = qu.params(n_classes=nc, cover=cover, labels=labels, bot=date(1995, 1, 1).toordinal(), mag_bands=0x7F)
        got = ctx.products(off, rows, dates, rfrawp=raw, cover=cname, labels=labels[:nc], bot=par.bot, mag_bands=0x7F)
        _same(got, qu.products(off, rows, dates, raw, par), (nc, cname, 'other parameters'))
        if nc > 1:
            assert want['lcsec'].any() and want['lcachg'].any()
    assert want['lcpri'].any() and want['sctime'].any()


def test_subsets_of_the_products(ctx, case100):
    """Any single product, lcachg without lcpri, and pairs: the bytes of the full request."""
    off, rows, dates, raw, want = case100
    full = want[abi.COVER_EXTEND]
    for n in qu.NAMES:
        got = ctx.products(off, rows, dates, rfrawp=raw, want=(n,))
        _same(got, {n: full[n]}, n)
    _same(ctx.products(off, rows, dates, rfrawp=raw, want='lcachg'), {'lcachg': full['lcachg']}, 'a name alone')
    assert full['lcachg'].any()
    for pair in (('scmag', 'lcsconf'), ('lcachg', 'sclast'), ('scmqa', 'lcpri')):
        _same(ctx.products(off, rows, dates, rfrawp=raw, want=pair), {n: full[n] for n in pair}, pair)
    with pytest.raises(ValueError, match='unknown product'):
        ctx.products(off, rows, dates, want=('sctime', 'lcnone'))
    with pytest.raises(ccdgpu.CcdGpuError, match='rfrawp is NULL'):
        ctx.products(off, rows, dates, want=('lcpri',), n_classes=9)
    with pytest.raises(ccdgpu.CcdGpuError, match='no product is requested'):
        ctx.products(off, rows, dates, want=())
    with pytest.raises(ccdgpu.CcdGpuError, match=r'dates\[0\]'):
        ctx.products(off, rows, [0])


def test_slab_independence(case100):
    """Contexts that keep 1, 7 and 64 pixels on the device at a time give the bytes of the default
    (and of the restatement): a value does not depend on how pixels are slabbed."""
    off, rows, dates, raw, want = case100
    results = {}
    old = os.environ.get('CCDGPU_PRODUCT_SLAB_PIXELS')
    try:
        for slab in (None, '1', '7', '64'):
            os.environ.pop('CCDGPU_PRODUCT_SLAB_PIXELS', None)
            if slab is not None:
                os.environ['CCDGPU_PRODUCT_SLAB_PIXELS'] = slab
            c = ccdgpu.Context(0)
            try:
                results[slab] = [c.products(off, rows, dates, rfrawp=raw, cover=cname) for cname, _ in COVERS]
                if slab == '7':
                    results['7 subset'] = c.products(off, rows, dates, rfrawp=raw, want=('lcachg', 'scmag'))
            finally:
                c.close()
    finally:
        os.environ.pop('CCDGPU_PRODUCT_SLAB_PIXELS', None)
        if old is not None:
            os.environ['CCDGPU_PRODUCT_SLAB_PIXELS'] = old
    for slab in ('1', '7', '64'):
        for got, first in zip(results[slab], results[None]):
            _same(got, first, slab)
    for got, (_, cover) in zip(results[None], COVERS):
        _same(got, want[cover], 'default context')
    _same(results['7 subset'], {n: want[abi.COVER_EXTEND][n] for n in ('lcachg', 'scmag')}, 'slabbed subset')


def test_caller_buffers(ctx, case100):
    """out arrays of the caller's (page-locked, reused) receive the same bytes."""
    off, rows, dates, raw, want = case100
    out = {n: ccdgpu.pinned_empty((33, 100), abi.PRODUCT_DTYPES[n]) for n in ('sctime', 'scmag', 'lcpri')}
    for cname, cover in COVERS:
        for a in out.values():
            a[...] = 7
        got = ctx.products(off, rows, dates, rfrawp=raw, cover=cname, want=('sctime', 'scmag', 'lcpri', 'lcachg'), out=out)
        assert all(got[n] is out[n] for n in out) and set(got) == set(out) | {'lcachg'}
        _same({n: np.asarray(a) for n, a in got.items()}, {n: want[cover][n] for n in got}, cname)
    for bad in (np.empty((33, 100), np.int16), np.empty((33, 99), np.uint16), np.empty((100, 33), np.uint16).T):
        with pytest.raises(ValueError, match=r"out\['sctime'\] must be"):
            ctx.products(off, rows, dates, out={'sctime': bad})


def test_sqrt_is_correctly_rounded(ctx):
    """10^5 sums of squares s through the device's sqrt: bytes against numpy's.  A sum reaches the
    device only as squares of float32 magnitudes, so each s is built from them (products_util.sqrt_mags):
    one-band sums -- perfect squares, from the denormals' squares to FLT_MAX's -- under a single
    mag_bands bit; a perfect square plus a second band's square of about a unit in its last place, its
    double neighbours; and general sums.  One-row tables whose row is the break of the date's year."""
    n = 16667
    t = date(2001, 7, 1).toordinal()
    rows = np.zeros(n, dtype=abi.ROW_DTYPE)
    rows['sday'], rows['eday'], rows['bday'] = t - 400, t - 30, t - 29
    rows['has_model'], rows['chprob'] = 1, 1.0
    rows['mag'] = qu.sqrt_mags(77, n)
    off = np.arange(n + 1, dtype=np.int64)
    total = 0
    for mask in qu.SQRT_MASKS:
        want = qu.records(rows, None, qu.params(mag_bands=mask)).scmag
        got = ctx.products(off, rows, [t], mag_bands=mask, want=('scmag',))['scmag']
        assert got.shape == (1, n) and got.dtype == np.float32
        assert got[0].tobytes() == want.tobytes(), (hex(mask), int((got[0].view(np.uint32) != want.view(np.uint32)).sum()))
        total += n
    assert total >= 10 ** 5
    one = qu.records(rows, None, qu.params(mag_bands=0x01)).scmag
    np.testing.assert_array_equal(one, np.abs(rows['mag'][:, 0]))  # (the root of a float32's square is the float32)
    assert np.isinf(one).any() and (one == 0).any() and (one[np.isfinite(one)] > 1e38).any() and (one[one > 0] < 1e-38).any()


def _forest(seed, n_classes):
    return Forest.from_arrays(*forest_util.random_forest(seed, 20, 5, 33, n_classes).args())


def _dense_chips():
    """Two change-dense generated chips of 64 pixels (smoke()'s kind), the first with one all-fill
    pixel: no clear observation, no segment, pyccd.default's row."""
    chips = [list(synth.chip(synth.config(5), 3, 0, 64)), list(synth.chip(synth.config(3), 1, 64, 64))]
    chips[0][2] = chips[0][2].copy()
    chips[0][1] = chips[0][1].copy()
    chips[0][2][5, :] = 1
    chips[0][1][:, 5, :] = -9999
    return [tuple(c) for c in chips], [(-585, 2805), (2415, 2805)]


def test_chained_equals_table(ctx):
    """products_rows (the run's segments on the device) gives the bytes of products on fetch_rows'
    rows, and of the restatement: without an rfrawp, and with classify_rows' rfrawp of a small forest
    -- the pixel without segments, whose default row the segments do not have, included."""
    chips, locs = _dense_chips()
    dates = synthetic.annual_dates(1985, 2017)
    batch = ctx.stage_chips(chips)
    ctx.run()
    ctx.set_forest(_forest(43, 9))
    try:
        raw = ctx.classify_rows(np.random.default_rng(9).normal(size=(128, 5)))
        at = 0
        for c, (cx, cy) in enumerate(locs):
            off, rows, _ = ctx.fetch_rows(c, cx, cy)
            n = ctx.chip_row_count(c)
            assert n == rows.shape[0] > 64
            rf, at = raw[at:at + n], at + n
            if c == 0:
                assert rows['has_model'][off[5]] == 0 and off[6] - off[5] == 1 and np.isnan(rf[off[5]]).all()
            for cname, cover in COVERS:
                want = ctx.products(off, rows, dates, rfrawp=rf, cover=cname)
                _same(ctx.products_rows(c, dates, rfrawp=rf, cover=cname), want, (c, cname))
                _same(want, qu.products(off, rows, dates, rf, qu.params(n_classes=9, cover=cover)), (c, cname, 'restatement'))
                _same(ctx.products_rows(c, dates, cover=cname), {k: want[k] for k in abi.CHANGE_PRODUCTS}, (c, cname, 'change'))
            _same(ctx.products_rows(c, dates, rfrawp=rf, want=('lcachg',)), {'lcachg': ctx.products(off, rows, dates, rfrawp=rf)['lcachg']}, c)
            assert want['lcpri'].any() and want['scstab'].any()
            if c == 0:  # the change-dense chip; its pixel 5 has no segment: no cover, no change, the stability period counted from the beginning of time
                assert want['sctime'].any() and want['scmag'].any() and want['lcachg'].any()
                assert not want['lcpri'][:, 5].any() and not want['sclast'][:, 5].any()
                np.testing.assert_array_equal(want['scstab'][:, 5], dates - abi.PRODUCT_BOT)
            with pytest.raises(ValueError, match='rfrawp has'):
                ctx.products_rows(c, dates, rfrawp=rf[:-1])
        assert at == raw.shape[0]
        with pytest.raises(ccdgpu.CcdGpuError, match='outside'):
            ctx.products_rows(2, dates)
        assert ctx.products_rows(1, [], want=('sctime',))['sctime'].shape == (0, 64)
    finally:
        ctx.clear_forest()
    # refused while a detection is pending, and without a run
    ctx.stage_slot_chips(0, batch)
    ctx.run_slot_begin(0)
    try:
        for call in (lambda: ctx.products_rows(0, dates), lambda: ctx.products(off, rows, dates), lambda: ctx.chip_row_count(0)):
            with pytest.raises(ccdgpu.CcdGpuError, match='not finished'):
                call()
    finally:
        ctx.run_slot_end()
    c2 = ccdgpu.Context(0)
    try:
        with pytest.raises(ccdgpu.CcdGpuError, match='no completed run'):
            c2.products_rows(0, dates)
    finally:
        c2.close()


def test_annual_chips_equals_the_tables(ctx):
    """ccdc.products.annual_chips (chipmunk chips in, detection, classification and products behind
    it) against products.annual over the segment tables classify_chips_tables gives for the same
    chips; a plane of a chip scatters into its raster by its keys."""
    from ccdc import chipmunk, randomforest
    (d, s, q), = [synth.chip(synth.config(5), 3, 0, 64)]
    order = np.argsort(d)[::-1]
    wire = chipmunk.chip_response(-585, 2805, d[order], s[:, :, order].copy(), q[:, order].copy())
    forest = _forest(44, 4)
    aux = np.random.default_rng(10).normal(size=(64, 5))
    dates = synthetic.annual_dates(1985, 2017)
    (key, got), = products.annual_chips(wire, dates, aux_of=lambda cx, cy: aux, forest=forest, context=ctx, labels=[11, 12, 13, 14])
    (key2, tabs), = randomforest.classify_chips_tables(wire, lambda cx, cy: aux, forest, context=ctx)
    keys, want = products.annual(tabs['segment'], dates, labels=[11, 12, 13, 14], context=ctx)
    assert key == key2 == (-585, 2805) and keys.shape == (64, 4)
    _same(got, want, 'annual_chips')
    assert set(np.unique(got['lcpri']).tolist()) <= {0, 11, 12, 13, 14} and got['lcpri'].any()
    (key3, change), = products.annual_chips(wire, dates, context=ctx)
    _same(change, {n: want[n] for n in abi.CHANGE_PRODUCTS}, 'without a forest')
    r = products.rasters(keys, got['sclast'][20])[-585, 2805]  # (64 pixels: the start of the chip's first row)
    np.testing.assert_array_equal(r[0, :64], got['sclast'][20])
    assert not r[1:].any() and not r[0, 64:].any()
    ctx.clear_forest()
