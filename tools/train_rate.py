#!/usr/bin/env python3
"""Developer tool (GPU box): time of the device's random-forest training (ccd_train.hip through
Context.train_forest) at the reference's forest shape -- 500 trees of depth 5, 33 features, 9
classes -- over --rows rows, beside sklearn's RandomForestClassifier.fit with 16 threads on the same
host.  Prints one JSON line.

  device   Context.train_forest on the host matrix, bins from ccdc.randomforest.find_splits (32 bins):
           the kernels' device time (HIP events around the launches of every level) and the whole call
           (matrix up, one host round trip per level and tree group, forest out); find_splits' own
           host time is reported apart
  sklearn  fit(n_estimators, max_depth, max_features='sqrt', n_jobs) on the same rows -- exact (unbinned)
           splits, so the forests differ; the times stand beside each other, not the trees

Every timed call is repeated after a warm-up call; each ends in a device synchronise (the calls are
synchronous).  The best and the median of --reps repeats are reported.

    python tools/train_rate.py [--rows 100000] [--reps 3] [--out FILE]
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
from ccdc import randomforest  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=100000)
ap.add_argument('--trees', type=int, default=500)
ap.add_argument('--depth', type=int, default=5)
ap.add_argument('--features', type=int, default=33)
ap.add_argument('--classes', type=int, default=9)
ap.add_argument('--bins', type=int, default=32)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--jobs', type=int, default=16)
ap.add_argument('--out', default=None)
a = ap.parse_args()

rng = np.random.default_rng(0)
x = rng.normal(size=(a.rows, a.features)).astype(np.float32).astype(np.float64)
y = ((np.abs(x[:, :4]).sum(axis=1) * 3).astype(np.int64) % a.classes).astype(np.int32)

t0 = time.perf_counter()
edges = randomforest.find_splits(x, a.bins)
splits_s = time.perf_counter() - t0

ctx = ccdgpu.Context(0)
par = dict(n_classes=a.classes, n_trees=a.trees, max_depth=a.depth, seed=0)
forest = ctx.train_forest(x, y, edges, **par)  # warm-up: code objects
wall, kern = [], []
for _ in range(a.reps):
    t0 = time.perf_counter()
    forest = ctx.train_forest(x, y, edges, **par)
    wall.append(time.perf_counter() - t0)
    kern.append(ctx.train_seconds)
ctx.set_forest(forest)
acc = float((np.argmax(ctx.classify(x[:20000]), axis=1) == y[:20000]).mean())
ctx.close()

out = {'tool': 'train_rate', 'rows': a.rows, 'n_trees': forest.n_trees, 'max_depth': a.depth, 'n_nodes': forest.n_nodes,
       'n_features': a.features, 'n_classes': a.classes, 'max_bins': a.bins, 'reps': a.reps,
       'device': {'kernel_s': min(kern), 'kernel_s_median': float(np.median(kern)), 'call_s': min(wall),
                  'call_s_median': float(np.median(wall)), 'find_splits_s': splits_s,
                  'row_trees_per_s_kernel': a.rows * a.trees / min(kern), 'row_trees_per_s_call': a.rows * a.trees / min(wall),
                  'training_accuracy': acc}}

from sklearn.ensemble import RandomForestClassifier  # noqa: E402
x32 = x.astype(np.float32)
sk = []
for _ in range(max(1, a.reps // 2)):
    rf = RandomForestClassifier(n_estimators=a.trees, max_depth=a.depth, max_features='sqrt', random_state=0, n_jobs=a.jobs)
    t0 = time.perf_counter()
    rf.fit(x32, y)
    sk.append(time.perf_counter() - t0)
out['sklearn'] = {'n_jobs': a.jobs, 'fit_s': min(sk), 'row_trees_per_s': a.rows * a.trees / min(sk),
                  'training_accuracy': float((rf.predict(x32[:20000]) == y[:20000]).mean())}
out['sklearn_over_device'] = {'kernel': min(sk) / min(kern), 'call': min(sk) / min(wall),
                              'call_with_find_splits': min(sk) / (min(wall) + splits_s)}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(line + '\n')
