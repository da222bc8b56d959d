#!/usr/bin/env python3
"""Developer tool (GPU box): rate of the annual change and land-cover product rasters
(ccd_products.hip) on one generated C3 chip and one C5 chip of 10^4 pixels at 33 annual dates, all
ten products, the rfrawp from a small generated forest (Context.classify_rows) -- the table path
(Context.products, the fetched rows and rfrawp uploaded), the chained path (Context.products_rows, the
run's segments on the device) and the chained path into page-locked arrays of the caller's -- against
the same evaluation by the numpy restatement of the rule (tests/products_util.py) on the host.
Prints one JSON line.

For every case: the kernels' device time (HIP events around the two launches) and the whole call
(host clock; the calls are synchronous and end in a stream synchronise: dates, offsets and rfrawp
up -- and the rows on the table path -- ten planes down), with the bytes each moves.  The output is
17 bytes per pixel and date.  Every timed call is repeated after a warm-up call; the best and the
median of --reps repeats are reported.  The device's planes are compared with the restatement's
(bytes).

    python tools/products_rate.py [--pixels 10000] [--configs 3 5] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'lcmap-firebird_amd'), os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402
import ccdgpu  # noqa: E402
import forest_util  # noqa: E402
import products_util  # noqa: E402
from ccdgpu import abi, synth  # noqa: E402
from ccdc import synthetic  # noqa: E402
from ccdc.randomforest import Forest  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--pixels', type=int, default=10000)
ap.add_argument('--configs', type=int, nargs='+', default=[3, 5])
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--classes', type=int, default=9)
ap.add_argument('--out', default=None)
a = ap.parse_args()


def timed(fn, reps):
    """(best, median) wall seconds and the matching kernel seconds of fn() -> kernel seconds."""
    fn()  # warm-up: code objects, buffers
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        k = fn()
        wall.append(time.perf_counter() - t0)
        kern.append(k)
    return min(wall), float(np.median(wall)), min(kern), float(np.median(kern))


dates = synthetic.annual_dates(1985, 2017)
n = dates.shape[0]
per_pixel_date = sum(np.dtype(t).itemsize for _, t in abi.PRODUCTS)
out = {'tool': 'products_rate', 'pixels': a.pixels, 'n_dates': int(n), 'reps': a.reps, 'n_classes': a.classes,
       'output_bytes_per_pixel_date': per_pixel_date, 'cases': {}}
ctx = ccdgpu.Context(0)
ctx.set_forest(Forest.from_arrays(*forest_util.random_forest(7, 50, 6, 33, a.classes).args()))
aux = np.random.default_rng(3).normal(size=(a.pixels, 5))
for cfg_id in a.configs:
    d, s, q = synth.chip(synth.config(cfg_id), 0, 0, a.pixels)
    ctx.stage_chips([(d, s, q)])
    detect_s = ctx.run()
    raw = ctx.classify_rows(aux)
    off, rows, _ = ctx.fetch_rows(0, 0, 0)
    output_bytes = a.pixels * n * per_pixel_date
    case = {'config': cfg_id, 'rows': int(rows.shape[0]), 'detect_kernel_s': detect_s, 'classify_kernel_s': ctx.forest_seconds,
            'output_bytes': output_bytes, 'table_upload_bytes': int(rows.nbytes + raw.nbytes + off.nbytes),
            'chained_upload_bytes': int(raw.nbytes + 2 * off.nbytes)}

    def table():
        ctx.products(off, rows, dates, rfrawp=raw)
        return ctx.products_seconds

    def chained():
        ctx.products_rows(0, dates, rfrawp=raw)
        return ctx.products_seconds

    pinned = {name: ccdgpu.pinned_empty((n, a.pixels), t) for name, t in abi.PRODUCTS}

    def chained_pinned():  # the chained path into page-locked arrays of the caller's, reused
        ctx.products_rows(0, dates, rfrawp=raw, out=pinned)
        return ctx.products_seconds

    for path, fn in (('table', table), ('chained', chained), ('chained_pinned', chained_pinned)):
        w, wm, k, km = timed(fn, a.reps)
        case[path] = {'kernel_s': k, 'kernel_s_median': km, 'call_s': w, 'call_s_median': wm,
                      'kernel_output_bytes_per_s': output_bytes / k, 'call_output_bytes_per_s': output_bytes / w,
                      'pixel_dates_per_s_kernel': a.pixels * n / k, 'pixel_dates_per_s_call': a.pixels * n / w}
    got = ctx.products_rows(0, dates, rfrawp=raw)
    t0 = time.perf_counter()
    ref = products_util.products(off, rows, dates, raw, products_util.params(n_classes=a.classes))
    host_s = time.perf_counter() - t0
    case['numpy_host'] = {'call_s': host_s, 'pixel_dates_per_s': a.pixels * n / host_s,
                          'planes_differing_from_device': [k for k in ref if ref[k].tobytes() != got[k].tobytes()]}
    case['device_over_numpy'] = {p: host_s / case[p]['call_s'] for p in ('table', 'chained', 'chained_pinned')}
    case['nonzero_share'] = {k: float(np.count_nonzero(got[k]) / got[k].size) for k in got}
    del pinned
    out['cases']['c%d' % cfg_id] = case
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(line + '\n')
