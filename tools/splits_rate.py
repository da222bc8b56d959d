#!/usr/bin/env python3
"""Developer tool (GPU box): time of the device's bin edges (ccd_splits.hip through
Context.find_splits) at the reference's shape -- 33 features, 32 bins -- over --rows rows, beside the
host rule (ccdc.randomforest.find_splits, a sort per column) on the same rows in the same process and
beside the training call the edges feed (Context.train_forest: 500 trees of depth 5, 9 classes).
Prints one JSON line.

  device   Context.find_splits on the host matrix: the kernels' device time (HIP events around the
           launches) and the whole call (buffers, matrix up, one round trip for the digit counts,
           edges out)
  host     ccdc.randomforest.find_splits(x, bins) on the same rows; the edges are compared, array_equal
  train    Context.train_forest with those edges: the whole call and its kernels

Every timed call is repeated after a warm-up call; each is synchronous.  The median and the best of
--reps repeats are reported (--host-reps for the host rule, which takes seconds).

    python tools/splits_rate.py [--rows 100000] [--reps 5] [--out FILE]

With --kernels-from DB the tool runs nothing: it turns the rocpd database of a kernel-trace run of its
own (rocprofv3 --kernel-trace --stats -- python tools/splits_rate.py --rows N --device-only) into the
per-kernel record, the share of each kernel of ccd_splits.hip in their total.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'lcmap-firebird_amd')]

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=100000)
ap.add_argument('--features', type=int, default=33)
ap.add_argument('--bins', type=int, default=32)
ap.add_argument('--trees', type=int, default=500)
ap.add_argument('--depth', type=int, default=5)
ap.add_argument('--classes', type=int, default=9)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--host-reps', type=int, default=5)
ap.add_argument('--device-only', action='store_true', help='only the device calls (for a kernel-trace run)')
ap.add_argument('--kernels-from', default=None, help='a rocpd database of a kernel-trace run: write its per-kernel record')
ap.add_argument('--out', default=None)
a = ap.parse_args()


def emit(out):
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if a.kernels_from:
    import re
    import sqlite3
    per = {}
    for name, start, end in sqlite3.connect(a.kernels_from).execute('select name, start, end from kernels'):
        m = re.search(r'ccd_splits_[a-z_]+', name)  # (lower case throughout: a mangled name's argument list begins with E)
        if m:
            per.setdefault(m.group(0), []).append((end - start) * 1e-6)
    total = sum(sum(d) for d in per.values())
    emit({'tool': 'rocprofv3 --kernel-trace --stats, a run of its own', 'workload':
          '%d calls of Context.find_splits (a warm-up and %d repeats), %d rows, %d features, %d bins'
          % (a.reps + 1, a.reps, a.rows, a.features, a.bins),
          'kernels': [{'kernel': k, 'launches': len(d), 'total_ms': round(sum(d), 3), 'mean_ms': round(sum(d) / len(d), 4),
                       'max_ms': round(max(d), 4), 'share': round(sum(d) / total, 4)}
                      for k, d in sorted(per.items(), key=lambda kv: -sum(kv[1]))],
          'total_ms': round(total, 3)})
    sys.exit(0)

import numpy as np  # noqa: E402
import ccdgpu  # noqa: E402
from ccdc import randomforest  # noqa: E402

rng = np.random.default_rng(0)
x = rng.normal(size=(a.rows, a.features)).astype(np.float32).astype(np.float64)  # (the matrix of tools/train_rate.py)
y = ((np.abs(x[:, :4]).sum(axis=1) * 3).astype(np.int64) % a.classes).astype(np.int32)

ctx = ccdgpu.Context(0)
edges = ctx.find_splits(x, a.bins)  # warm-up: code objects
wall, kern = [], []
for _ in range(a.reps):
    t0 = time.perf_counter()
    edges = ctx.find_splits(x, a.bins)
    wall.append(time.perf_counter() - t0)
    kern.append(ctx.splits_seconds)
out = {'tool': 'splits_rate', 'rows': a.rows, 'n_features': a.features, 'max_bins': a.bins, 'reps': a.reps,
       'n_edges': [int(e.shape[0]) for e in edges],
       'device': {'kernel_s_median': float(np.median(kern)), 'kernel_s': min(kern), 'call_s_median': float(np.median(wall)),
                  'call_s': min(wall)}}
if not a.device_only:
    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ref = randomforest.find_splits(x, a.bins)
        host.append(time.perf_counter() - t0)
    out['host'] = {'reps': a.host_reps, 'find_splits_s_median': float(np.median(host)), 'find_splits_s': min(host),
                   'edges_equal': bool(len(ref) == len(edges) and all(np.array_equal(u, v) for u, v in zip(ref, edges)))}
    par = dict(n_classes=a.classes, n_trees=a.trees, max_depth=a.depth, seed=0)
    ctx.train_forest(x, y, edges, **par)  # warm-up
    twall, tkern = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.train_forest(x, y, edges, **par)
        twall.append(time.perf_counter() - t0)
        tkern.append(ctx.train_seconds)
    out['train'] = {'n_trees': a.trees, 'max_depth': a.depth, 'n_classes': a.classes, 'call_s_median': float(np.median(twall)),
                    'call_s': min(twall), 'kernel_s_median': float(np.median(tkern))}
    d, h, t = out['device']['call_s_median'], out['host']['find_splits_s_median'], out['train']['call_s_median']
    out['ratios'] = {'host_over_device_call': h / d, 'device_call_over_train_call': d / t,
                     'train_with_host_splits_s': h + t, 'train_with_device_splits_s': d + t,
                     'end_to_end_speedup': (h + t) / (d + t)}
ctx.close()
emit(out)
