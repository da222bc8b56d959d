#!/usr/bin/env python3
"""Developer tool (GPU box): kernel time of the out-of-bag permutation counts (ccd_forest_permutation in
ccd_forest.hip) beside the out-of-bag walk's (ccd_forest_oob) on the same rows and the same forest, in
one process.  The forest is trained on the device at the reference's shape -- 500 trees of depth 5, 9
classes, 33 features -- over --train-rows rows; both kernels then take --rows rows (10^6) with labels by
the training set's formula.  Done plainly the counts are n_features + 1 out-of-bag walks; the kernel
walks a (row, tree) pair once and again only for the features on its path, and the run fails (exit 1)
unless its time is below (n_features + 1) times the out-of-bag kernel's.  Prints one JSON line.

Pairs hashed = rows x trees; base walks = the out-of-bag pairs (the sum of oob_rows); re-walks = the
distinct features on the paths of those pairs, counted on the host over the first --count-rows rows
(numpy) and scaled by the base walks.

Every timed call is repeated after a warm-up call; each ends in a device synchronise (the calls are
synchronous).  The best and the median of --reps repeats are reported.

    python tools/permutation_rate.py [--rows 1000000] [--reps 5] [--out FILE]
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
ap.add_argument('--count-rows', type=int, default=20000)
ap.add_argument('--trees', type=int, default=500)
ap.add_argument('--depth', type=int, default=5)
ap.add_argument('--classes', type=int, default=9)
ap.add_argument('--seed', type=int, default=0)
ap.add_argument('--perm-seed', type=int, default=0)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=None)
a = ap.parse_args()


def labels(m):
    return ((np.abs(m[:, :4]).sum(axis=1) * 3).astype(np.int64) % a.classes).astype(np.int32)


rng = np.random.default_rng(0)
xt = rng.normal(size=(a.train_rows, 33)).astype(np.float32).astype(np.float64)
x = rng.normal(size=(a.rows, 33)).astype(np.float32).astype(np.float64)
y = labels(x)

ctx = ccdgpu.Context(0)
forest = ctx.train_forest(xt, labels(xt), randomforest.find_splits(xt, 32), n_classes=a.classes, n_trees=a.trees,
                          max_depth=a.depth, seed=a.seed)
ctx.set_forest(forest)


def timed(fn, reps):
    """(best, median) kernel seconds of fn() -> kernel seconds, after one warm-up call."""
    fn()  # warm-up: code objects, buffers
    k = [fn() for _ in range(reps)]
    return min(k), float(np.median(k))


state = {}


def oob():
    state['n'] = ctx.forest_oob(x, a.seed)[1]
    return ctx.oob_seconds


def permutation():
    state['counts'] = ctx.forest_permutation(x, y, a.seed, a.perm_seed)
    return ctx.permutation_seconds


def path_features(rows):
    """The distinct features on the paths of the out-of-bag (row, tree) pairs of the first ``rows`` rows, and
    those pairs."""
    m = x[:rows]
    walks = features = 0
    r = np.arange(rows, dtype=np.uint64)
    golden = np.uint64(0x9E3779B97F4A7C15)

    def mix(z):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    with np.errstate(over='ignore'):
        key = mix(np.uint64(a.seed) + golden)
        for t, root in enumerate(forest.root.tolist()):
            u = mix(mix(mix(key + golden + np.uint64(t)) + golden + r) + golden) >> np.uint64(32)
            idx = np.nonzero(u < np.uint64(ccdgpu.abi.OOB_CUT))[0]
            node = np.full(idx.shape[0], root, dtype=np.int64)
            mask = np.zeros(idx.shape[0], dtype=np.uint64)
            walks += idx.shape[0]
            while True:
                go = np.nonzero(forest.feature[node] >= 0)[0]
                if go.size == 0:
                    break
                at = node[go]
                f = forest.feature[at]
                mask[go] |= np.uint64(1) << f.astype(np.uint64)
                node[go] = np.where(m[idx[go], f] <= forest.threshold[at], forest.left[at], forest.right[at])
            features += int(sum(int(((mask >> np.uint64(b)) & np.uint64(1)).sum()) for b in range(33)))
    return features, walks


ok, okm = timed(oob, a.reps)
pk, pkm = timed(permutation, a.reps)
oob_rows, correct, lost, gained = state['counts']
base_walks = int(oob_rows.sum())
assert base_walks == int(state['n'].sum())
feats, walks = path_features(min(a.count_rows, a.rows))
s = randomforest.permutation_summary(oob_rows, correct, lost, gained)
nf = forest.n_features
out = {'tool': 'permutation_rate', 'rows': a.rows, 'n_trees': forest.n_trees, 'max_depth': forest.max_depth,
       'n_nodes': forest.n_nodes, 'n_classes': forest.n_classes, 'n_features': nf, 'reps': a.reps,
       'train_rows': a.train_rows, 'threads': int(ccdgpu.lib().ccdk_forest_threads(nf)),
       'oob': {'kernel_s': ok, 'kernel_s_median': okm},
       'permutation': {'kernel_s': pk, 'kernel_s_median': pkm, 'pairs_hashed': a.rows * forest.n_trees,
                       'base_walks': base_walks, 'rewalks_per_base_walk': feats / float(walks),
                       'rewalks_counted_over_rows': min(a.count_rows, a.rows),
                       'rewalks_estimated': int(round(base_walks * feats / float(walks))),
                       'correct': int(correct.sum()), 'lost': int(lost.sum()), 'gained': int(gained.sum())},
       'plain_form_kernel_s': (nf + 1) * ok, 'permutation_over_oob_kernel_s': pk / ok,
       'permutation_over_plain_form': pk / ((nf + 1) * ok),
       'importances_top5': [[int(f), float(s.importances[f])] for f in np.argsort(s.importances)[::-1][:5]]}
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, 'w') as fh:
        fh.write(line + '\n')
if not pk < (nf + 1) * ok:
    sys.exit('the permutation kernel (%.4g s) is not below %d out-of-bag walks (%.4g s): the path mask bought nothing'
             % (pk, nf + 1, (nf + 1) * ok))
