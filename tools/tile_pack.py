#!/usr/bin/env python3
"""Tile leg with the band runs bit-packed and not (developer tool, GPU box): the runner's tile
path (ccdc.runner.changedetection over ccdgpu.synth.TileSource pool chips, as bench.py's tile leg
runs it) with EncodingSource(pack=False / True) for drop = 'unread' and 'lossless', the four
variants interleaved ``--reps`` times over the same chips.  Per run: pixels/s, sent_over_raw, the
encoder's thread-seconds (EncodingSource.encode_seconds, wall time of the fetch threads' encode
calls) and the process's CPU seconds; the JSON goes to ``--out`` (profiles/).

usage: tile_pack.py [--chips 300] [--reps 3] [--config 3] [--out profiles/pack/tile_pack.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lcmap-firebird_amd'))
import ccdgpu  # noqa: E402
from ccdc import runner  # noqa: E402
from ccdgpu import synth  # noqa: E402

TILE_CHIPS = 2500


class Kept(object):
    """a context lent to the runner (its close() at the end of a tile is a no-op)"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def close(self):
        pass


class Offset(object):
    """a source whose positions are shifted (the warm-up's chips)"""

    def __init__(self, src, off):
        self.src, self.off = src, off

    def __call__(self, positions):
        return self.src([p + self.off for p in positions])

    @property
    def has_views(self):
        return getattr(self.src, 'has_views', hasattr(self.src, 'views'))

    def views(self, positions):
        return self.src.views([p + self.off for p in positions])

    def release(self, batch):
        self.src.release(batch)


def xy(p):
    t, c = divmod(p % 1000000, TILE_CHIPS)
    return (-1815585 + 3000 * (c // 50) + 150000 * t, 1064805 - 3000 * (c % 50))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chips', type=int, default=300)
    ap.add_argument('--warm', type=int, default=48)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--config', type=int, default=3)
    ap.add_argument('--pool', type=int, default=32)
    ap.add_argument('--contexts', type=int, default=4)
    ap.add_argument('--batch', type=int, default=6)
    ap.add_argument('--threads', type=int, default=3)
    ap.add_argument('--depth', type=int, default=2)
    ap.add_argument('--copy-cus', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pack', 'tile_pack.json'))
    args = ap.parse_args()
    device = 0
    cfg = synth.config(args.config)
    runner.bind_to_device_node(device, ccdgpu.device_numa_node(device))
    src = synth.TileSource(cfg, device=device, batch_chips=args.batch, mode='pool', pool_chips=args.pool,
                           rotate_threads=args.threads)
    src.prepare()
    n_inflight = args.contexts * (args.depth + 1) + 1
    variants = [(drop, pack) for drop in ('unread', 'lossless') for pack in (False, True)]
    esrcs = {}
    for drop, pack in variants:
        e = esrcs[(drop, pack)] = runner.EncodingSource(src, threads=args.threads, drop=drop, pack=pack)
        e.prefill(n_inflight, args.batch, 10000, src.max_obs)
    ctxs = [ccdgpu.Context(device, copy_cus=args.copy_cus) for _ in range(args.contexts)]

    def run(n, source):
        lent = iter(ctxs)
        sink = runner.SummarySink(digest=False)
        return runner.changedetection([xy(p) for p in range(n)], source, device=device, contexts=args.contexts,
                                      batch_chips=args.batch, sink=sink, upload_depth=args.depth,
                                      context_factory=lambda dev: Kept(next(lent)), encode=False)

    runs = []
    for drop, pack in variants:  # warm every variant (first launches, buffer growth) outside the timing
        run(args.warm, Offset(esrcs[(drop, pack)], 1000000))
    for rep in range(args.reps):
        for drop, pack in variants:
            e = esrcs[(drop, pack)]
            ctxs[0].synchronize()
            b0 = (e.bytes_raw, e.bytes_sent, e.encode_seconds)
            c0, t0 = time.process_time(), time.perf_counter()
            res = run(args.chips, e)
            ctxs[0].synchronize()
            el, cpu = time.perf_counter() - t0, time.process_time() - c0
            px = sum(c['n_pix'] for c in res['chips'])
            raw_b, sent_b = e.bytes_raw - b0[0], e.bytes_sent - b0[1]
            r = {'rep': rep, 'drop': drop, 'pack': pack, 'pixels_per_s': round(px / el, 1), 'seconds': round(el, 4),
                 'pixels': px, 'sent_over_raw': round(sent_b / raw_b, 4), 'upload_bytes_raw': raw_b,
                 'upload_bytes_sent': sent_b, 'sent_gbs': round(sent_b / el / 1e9, 2),
                 'encode_thread_seconds': round(e.encode_seconds - b0[2], 3), 'process_cpu_seconds': round(cpu, 3)}
            runs.append(r)
            print(json.dumps(r), flush=True)
    for c in ctxs:
        c.close()
    for e in esrcs.values():
        e.close()
    src.close()
    summary = {}
    for drop, pack in variants:
        rs = [r for r in runs if r['drop'] == drop and r['pack'] == pack]
        key = '%s_%s' % (drop, 'packed' if pack else 'mode1')
        summary[key] = {k: sorted(r[k] for r in rs)[len(rs) // 2]
                        for k in ('pixels_per_s', 'sent_over_raw', 'encode_thread_seconds', 'process_cpu_seconds', 'sent_gbs')}
        summary[key]['pixels_per_s_all'] = [r['pixels_per_s'] for r in rs]
    out = {'tool': 'tools/tile_pack.py', 'args': vars(args), 'encoder_avx512_vbmi2': bool(ccdgpu.encode_vector_path()),
           'omp_num_threads_env': os.environ.get('OMP_NUM_THREADS'), 'median_of_reps': summary, 'runs': runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
