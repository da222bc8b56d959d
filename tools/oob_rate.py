#!/usr/bin/env python3
"""Developer tool (GPU box): kernel time of the out-of-bag walk (ccd_forest_oob in ccd_forest.hip)
beside the classification kernel's (ccd_forest_classify) on the same rows and the same forest, in one
process.  The forest is trained on the device at the reference's shape -- 500 trees of depth 5, 9
classes, 33 features -- over --train-rows rows; both kernels then take --rows rows (10^6) of the
host-matrix path.  The out-of-bag walk hashes every (row, tree) pair and walks about exp(-1) = 37 % of
them; the classification walks all of them.  Prints one JSON line.

Every timed call is repeated after a warm-up call; each ends in a device synchronise (the calls are
synchronous).  The best and the median of --reps repeats are reported.

    python tools/oob_rate.py [--rows 1000000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'lcmap-firebird_amd')]
import numpy as np  # noqa: E402
import ccdgpu  # noqa: E402
from ccdc import randomforest  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=1000000)
ap.add_argument('--train-rows', type=int, default=20000)
ap.add_argument('--trees', type=int, default=500)
ap.add_argument('--depth', type=int, default=5)
ap.add_argument('--classes', type=int, default=9)
ap.add_argument('--seed', type=int, default=0)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=None)
a = ap.parse_args()

rng = np.random.default_rng(0)
xt = rng.normal(size=(a.train_rows, 33)).astype(np.float32).astype(np.float64)
yt = ((np.abs(xt[:, :4]).sum(axis=1) * 3).astype(np.int64) % a.classes).astype(np.int32)
x = rng.normal(size=(a.rows, 33)).astype(np.float32).astype(np.float64)

ctx = ccdgpu.Context(0)
forest = ctx.train_forest(xt, yt, randomforest.find_splits(xt, 32), n_classes=a.classes, n_trees=a.trees,
                          max_depth=a.depth, seed=a.seed)
ctx.set_forest(forest)


def timed(fn, reps):
    """(best, median) kernel seconds of fn() -> kernel seconds, after one warm-up call."""
    fn()  # warm-up: code objects, buffers
    k = [fn() for _ in range(reps)]
    return min(k), float(np.median(k))


state = {}


def classify():
    ctx.classify(x)
    return ctx.forest_seconds


def oob():
    state['raw'], state['n'] = ctx.forest_oob(x, a.seed)
    return ctx.oob_seconds


ck, ckm = timed(classify, a.reps)
ok, okm = timed(oob, a.reps)
walked = int(state['n'].sum())
out = {'tool': 'oob_rate', 'rows': a.rows, 'n_trees': forest.n_trees, 'max_depth': forest.max_depth,
       'n_nodes': forest.n_nodes, 'n_classes': forest.n_classes, 'n_features': forest.n_features, 'reps': a.reps,
       'train_rows': a.train_rows, 'train_kernel_s': ctx.train_seconds,
       'classify': {'kernel_s': ck, 'kernel_s_median': ckm, 'kernel_rows_per_s': a.rows / ck,
                    'pairs_walked': a.rows * forest.n_trees},
       'oob': {'kernel_s': ok, 'kernel_s_median': okm, 'kernel_rows_per_s': a.rows / ok,
               'pairs_hashed': a.rows * forest.n_trees, 'pairs_walked': walked,
               'share_walked': walked / float(a.rows * forest.n_trees),
               'rows_unscored': int((state['n'] == 0).sum())},
       'oob_over_classify_kernel_s': ok / ck}
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, 'w') as fh:
        fh.write(line + '\n')
