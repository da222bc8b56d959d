#!/usr/bin/env python3
"""Developer tool (GPU box): rate of the prediction of band values (ccd_predict.hip) on one
generated C3 chip of 10^4 pixels -- the chained path (Context.predict_rows, the run's segments on
the device) and the table path (Context.predict, the fetched rows uploaded), int16 and float32
output, at the chip's own dates and at 33 annual dates -- against the same evaluation in numpy on
the host.  Prints one JSON line.

For every case: the kernels' device time (HIP events around the launches) and the whole call (host
clock; the calls are synchronous and end in a stream synchronise: dates and rows up, values and
row indices down), and the output bytes per second of each against the HBM and PCIe figures below.
The kernel writes 7 x (2 or 4) + 4 bytes per pixel and date and reads little else, so HBM write
bandwidth bounds it; the call then copies the same bytes to the host: into new pageable arrays
(chained, table) or into page-locked arrays of the caller's that are reused (chained_pinned).

Every timed call is repeated after a warm-up call.  The best and the median of --reps repeats are
reported.

    python tools/predict_rate.py [--pixels 10000] [--config 3] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'lcmap-firebird_amd')]
import numpy as np  # noqa: E402
import ccdgpu  # noqa: E402
from ccdgpu import synth  # noqa: E402
from ccdc import synthetic  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, specification
HBM_MEASURED = 6.29e12  # bytes/s, float4 copy
PCIE_PEAK = 63e9       # bytes/s, PCIe Gen5 x16 specification

ap = argparse.ArgumentParser()
ap.add_argument('--pixels', type=int, default=10000)
ap.add_argument('--config', type=int, default=3)
ap.add_argument('--reps', type=int, default=5)
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


def numpy_predict(off, rows, dates, dtype):
    """The rule of include/ccdgpu.h in numpy (cover 'span'), as a caller without the device path
    evaluates a fetched table: basis once, every row over the dates its span holds."""
    t = np.asarray(dates, dtype=np.int64)
    w12 = 2.0 * np.pi / 365.2425 * t.astype(np.float64)
    B = np.stack([t.astype(np.float64), np.cos(w12), np.sin(w12), np.cos(2.0 * w12), np.sin(2.0 * w12), np.cos(3.0 * w12),
                  np.sin(3.0 * w12)], axis=1)
    n_pix = off.shape[0] - 1
    i16 = dtype == 'int16'
    out = np.full((7, n_pix, t.shape[0]), -9999 if i16 else np.nan, dtype=np.int16 if i16 else np.float32)
    pix = np.repeat(np.arange(n_pix), np.diff(off))
    free = np.ones((n_pix, t.shape[0]), dtype=bool)
    for j in range(rows.shape[0]):
        r = rows[j]
        if not r['has_model']:
            continue
        m = (t >= r['sday']) & (t <= r['eday']) & free[pix[j]]
        if not m.any():
            continue
        free[pix[j], m] = False
        v = r['intercept'].astype(np.float64)[:, None] + r['coef'].astype(np.float64) @ B[m].T
        out[:, pix[j], m] = np.clip(np.rint(v), -32768, 32767) if i16 else v
    return out


cfg = synth.config(a.config)
d, s, q = synth.chip(cfg, 0, 0, a.pixels)
ctx = ccdgpu.Context(0)
ctx.stage_chips([(d, s, q)])
detect_s = ctx.run()
off, rows, _ = ctx.fetch_rows(0, 0, 0)
cases = {'own_dates': np.ascontiguousarray(d, dtype=np.int64), 'annual_33': synthetic.annual_dates(1985, 2017)}
out = {'tool': 'predict_rate', 'config': a.config, 'pixels': a.pixels, 'rows': int(rows.shape[0]), 'reps': a.reps,
       'detect_kernel_s': detect_s, 'hbm_peak_bytes_per_s': HBM_PEAK, 'hbm_measured_bytes_per_s': HBM_MEASURED,
       'pcie_peak_bytes_per_s': PCIE_PEAK, 'cases': {}}

for name, dates in cases.items():
    n = dates.shape[0]
    for dtype in ('int16', 'float32'):
        esz = 2 if dtype == 'int16' else 4
        kernel_bytes = a.pixels * n * (7 * esz + 4)  # values and row indices written
        case = {'n_dates': int(n), 'dtype': dtype, 'output_bytes': kernel_bytes, 'table_rows_bytes': int(rows.nbytes)}

        def chained():
            ctx.predict_rows(0, dates, dtype=dtype)
            return ctx.predict_seconds

        def table():
            ctx.predict(off, rows, dates, dtype=dtype)
            return ctx.predict_seconds

        pin_out = ccdgpu.pinned_empty((7, a.pixels, n), np.int16 if dtype == 'int16' else np.float32)
        pin_idx = ccdgpu.pinned_empty((a.pixels, n), np.int32)

        def chained_pinned():  # the chained path into page-locked arrays of the caller's, reused
            ctx.predict_rows(0, dates, dtype=dtype, out=pin_out, seg_index=pin_idx)
            return ctx.predict_seconds

        for path, fn in (('chained', chained), ('table', table), ('chained_pinned', chained_pinned)):
            w, wm, k, km = timed(fn, a.reps)
            case[path] = {'kernel_s': k, 'kernel_s_median': km, 'call_s': w, 'call_s_median': wm,
                          'kernel_bytes_per_s': kernel_bytes / k, 'kernel_share_of_hbm_peak': kernel_bytes / k / HBM_PEAK,
                          'kernel_share_of_hbm_measured': kernel_bytes / k / HBM_MEASURED,
                          'call_bytes_per_s': kernel_bytes / w, 'call_share_of_pcie_peak': kernel_bytes / w / PCIE_PEAK,
                          'pixel_dates_per_s_kernel': a.pixels * n / k, 'pixel_dates_per_s_call': a.pixels * n / w}
        got = ctx.predict(off, rows, dates, dtype=dtype)[0]
        t0 = time.perf_counter()
        ref = numpy_predict(off, rows, dates, dtype)
        host_s = time.perf_counter() - t0
        if dtype == 'int16':
            diff = float(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max())
        else:
            both = ~np.isnan(got) & ~np.isnan(ref)
            diff = float(np.abs(got[both] - ref[both]).max()) if both.any() else 0.0
            case['fill_mismatches'] = int((np.isnan(got) != np.isnan(ref)).sum())
        case['numpy_host'] = {'call_s': host_s, 'pixel_dates_per_s': a.pixels * n / host_s, 'max_abs_diff_vs_device': diff}
        case['device_over_numpy'] = {'chained_call': host_s / case['chained']['call_s'], 'table_call': host_s / case['table']['call_s'],
                                     'chained_pinned_call': host_s / case['chained_pinned']['call_s']}
        del pin_out, pin_idx
        out['cases']['%s_%s' % (name, dtype)] = case
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(line + '\n')
