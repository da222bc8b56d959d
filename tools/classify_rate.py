#!/usr/bin/env python3
"""Developer tool (GPU box): rate of the random-forest classification (ccd_forest.hip) at the
reference's forest shape -- 500 trees of depth 5, 9 classes, 33 features -- against sklearn's
predict_proba with 16 threads on the same host.  Prints one JSON line.

  host-matrix path   Context.classify over --rows rows (10^6): the kernel's device time (HIP
                     events around the launches) and the whole call (host matrix in, predictions
                     out: 264 B up and 36 B down per row over PCIe)
  chained path       Context.classify_rows behind the detection of --chips synthetic chips: the
                     rows never leave the device; gather + forest kernels' device time, and the
                     whole call (aux up, predictions down)

Every timed call is repeated after a warm-up call; each ends in a device synchronise (the calls
are synchronous).  The best and the median of --reps repeats are reported.

    python tools/classify_rate.py [--rows 1000000] [--chips 8] [--reps 5] [--out FILE]
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
from ccdc.randomforest import Forest  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=1000000)
ap.add_argument('--trees', type=int, default=500)
ap.add_argument('--depth', type=int, default=5)
ap.add_argument('--classes', type=int, default=9)
ap.add_argument('--chips', type=int, default=8, help='10000-pixel chips of the chained path\'s batch (0: skip it)')
ap.add_argument('--config', type=int, default=3)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--jobs', type=int, default=16)
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


from sklearn.ensemble import RandomForestClassifier  # noqa: E402
rng = np.random.default_rng(0)
xt = rng.normal(size=(20000, 33)).astype(np.float32)
yt = (np.abs(xt[:, :4]).sum(axis=1) * 3).astype(np.int64) % a.classes
rf = RandomForestClassifier(n_estimators=a.trees, max_depth=a.depth, random_state=0, n_jobs=a.jobs).fit(xt, yt)
forest = Forest.from_sklearn(rf)
x = rng.normal(size=(a.rows, 33)).astype(np.float32).astype(np.float64)

ctx = ccdgpu.Context(0)
ctx.set_forest(forest)
out = {'tool': 'classify_rate', 'rows': a.rows, 'n_trees': forest.n_trees, 'max_depth': forest.max_depth,
       'n_nodes': forest.n_nodes, 'n_classes': forest.n_classes, 'n_features': forest.n_features, 'reps': a.reps}


def host_path():
    ctx.classify(x)
    return ctx.forest_seconds


w, wm, k, km = timed(host_path, a.reps)
out['host_matrix'] = {'rows': a.rows, 'kernel_s': k, 'kernel_s_median': km, 'call_s': w, 'call_s_median': wm,
                      'kernel_rows_per_s': a.rows / k, 'end_to_end_rows_per_s': a.rows / w,
                      'pcie_bytes_per_row': 33 * 8 + forest.n_classes * 4,
                      'end_to_end_gb_per_s': a.rows * (33 * 8 + forest.n_classes * 4) / w / 1e9}
got = ctx.classify(x[:20000])

# sklearn on the same host: predict_proba with n_jobs threads (float32 input, as sklearn converts)
x32 = x.astype(np.float32)
rf.set_params(n_jobs=a.jobs)
rf.predict_proba(x32[:20000])
sk = []
for _ in range(max(2, a.reps // 2)):
    t0 = time.perf_counter()
    proba = rf.predict_proba(x32)
    sk.append(time.perf_counter() - t0)
out['sklearn'] = {'n_jobs': a.jobs, 'call_s': min(sk), 'rows_per_s': a.rows / min(sk)}
out['max_abs_diff_vs_sklearn'] = float(np.abs(got / forest.n_trees - proba[:20000]).max())
out['device_over_sklearn'] = {'kernel': out['host_matrix']['kernel_rows_per_s'] / out['sklearn']['rows_per_s'],
                              'end_to_end': out['host_matrix']['end_to_end_rows_per_s'] / out['sklearn']['rows_per_s']}

if a.chips > 0:
    cfg = synth.config(a.config)
    batch = ccdgpu.ChipBatch.from_chips([synth.chip(cfg, c % 16, 0, 10000) for c in range(a.chips)])
    ctx.stage_chips(batch)
    det_s = ctx.run()
    aux = rng.normal(size=(batch.total_pixels, 5))

    def chained():
        ctx.classify_rows(aux)
        return ctx.forest_seconds

    w, wm, k, km = timed(chained, a.reps)
    n = ctx.forest_rows
    out['chained'] = {'chips': a.chips, 'pixels': batch.total_pixels, 'rows': n, 'detect_kernel_s': det_s,
                      'kernel_s': k, 'kernel_s_median': km, 'call_s': w, 'call_s_median': wm,
                      'kernel_rows_per_s': n / k, 'end_to_end_rows_per_s': n / w}
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, 'w') as fh:
        fh.write(line + '\n')
