"""bench.py's roofline bookkeeping on CPU: the committed PMC records (profiles/pmc_*.json) carry
the fields the bench line reads and are found by their workload keys, and the hardware FP64
fraction the bench reports is reproducible from a record and the committed kernel-stats average.
The plain run: its options, the arrays --dump-outputs writes, and (GPU) a small run end to end."""
import csv
import glob
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_writes_float64_arrays_ordered_by_position_and_pixel(tmp_path):
    import numpy as np
    from ccdgpu import abi
    rng = np.random.default_rng(7)

    def pixel(n_rows, words):
        r = np.zeros(n_rows, abi.ROW_DTYPE)
        r['px'] = rng.integers(-2 ** 31, 2 ** 31 - 1, n_rows)
        r['sday'] = np.arange(n_rows) + 700000
        r['chprob'] = rng.random(n_rows)
        r['coef'] = rng.standard_normal((n_rows, 7, 7))
        r['intercept'] = rng.standard_normal((n_rows, 7))
        return r, rng.integers(0, 2 ** 32, words, dtype=np.uint64).astype('<u4')

    samples, n_rows = {}, 0
    for pos, n_obs in ((9, 1421), (4, 2121)):  # (unordered on purpose)
        keep = {}
        for j, px in enumerate(bench.sample_pixels(pos, bench.DUMP_PIXELS + 3)):  # 3 pixels beyond the dump's
            keep[px] = pixel(1 + j % 3, (n_obs + 31) // 32)
        samples[pos] = (0, 0, n_obs, keep)
        n_rows += sum(keep[px][0].shape[0] for px in bench.sample_pixels(pos, bench.DUMP_PIXELS))
    chips = [{'pos': p, 'cx': 3000 * p, 'cy': -3000 * p, 'n_pix': 10000, 'n_obs': samples[p][2], 'rows': 12345 + p,
              'models': 11111 + p, 'digest': None} for p in (9, 4)]
    rec = bench.dump_outputs(str(tmp_path / 'out'), samples, chips)
    got = {n: np.load(str(tmp_path / 'out' / (n + '.npy'))) for n in rec['arrays']}
    assert sorted(got) == ['chip_summaries', 'mask_index', 'mask_words', 'row_index', 'rows']
    assert all(a.dtype == np.float64 for a in got.values())
    assert rec['bytes'] == sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES
    n_px = 2 * bench.DUMP_PIXELS
    assert got['rows'].shape == (n_rows, 78) and got['row_index'].shape == (n_rows, 2)
    assert got['mask_words'].shape == (n_px, 67) and got['mask_index'].shape == (n_px, 3)
    order = [tuple(x) for x in got['row_index']]
    assert order == sorted(order) and {int(p) for p, _ in order} == {4, 9}
    assert [tuple(x[:2]) for x in got['mask_index']] == sorted(set(order))
    # every value survives the conversion: the first row of the first pixel of position 4
    px = bench.sample_pixels(4, bench.DUMP_PIXELS)[0]
    r, m = samples[4][3][px]
    want = np.concatenate([np.asarray(r[0][f], dtype=np.float64).ravel() for f in abi.ROW_DTYPE.names])
    assert np.array_equal(got['rows'][0], want)
    assert np.array_equal(got['mask_words'][0].astype('<u4'), m)
    assert np.array_equal(got['mask_words'][n_px - 1][45:], np.zeros(22))  # 1421 obs: 45 words, padded
    assert got['chip_summaries'].tolist() == [[4, 12000, -12000, 10000, 2121, 12349, 11115],
                                              [9, 27000, -27000, 10000, 1421, 12354, 11120]]


def test_plain_run_options(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup, a.step_chips) == (False, None, 7, 2, 500)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--no-tile'])
    try:
        bench.parse()
    except SystemExit as e:
        assert e.code == 2  # the resident leg is part of --full
    else:
        raise AssertionError('--no-tile without --full was accepted')
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--no-tile', '--full'])
    assert bench.parse().no_tile


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_one(tmp_path, monkeypatch, capsys):
    """A small plain run in this process: 3 timed steps of 3 chips after 1 warmup step; the line
    carries the headline fields and no --full leg; the dump holds the last step's 3 chips."""
    import numpy as np
    out = str(tmp_path / 'dump')
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--step-chips', '3',
                                      '--tile-pool', '4', '--tile-batch', '1', '--tile-contexts', '2', '--tile-depth', '1',
                                      '--tile-no-numa', '--dump-outputs', out])
    bench.main()
    d = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert d['metric'].startswith('pixels/sec change-detected') and d['unit'] == 'pixels/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'f64' and d['steps'] == 3 and d['full'] is False
    t = d['tile']
    assert (t['chips'], t['chips_per_step'], t['pixels'], t['parity_sample']) == (9, 3, 90000, None)
    assert d['ms_per_step'] == pytest.approx(t['seconds'] * 1e3 / 3)
    assert d['value'] == pytest.approx(t['pixels'] / t['seconds'])
    assert d['roofline'] is None and 'resident' not in d and 'cpu_baseline' not in d and 'tile_lossless' not in d
    got = {n: np.load(os.path.join(out, n + '.npy')) for n in d['outputs_dumped']['arrays']}
    assert got['chip_summaries'][:, 0].tolist() == list(range(6, 9))
    assert sorted(set(got['row_index'][:, 0].tolist())) == list(range(6, 9))
    assert got['mask_index'].shape[0] == 3 * bench.DUMP_PIXELS and got['rows'].shape[1] == 78
    assert got['rows'].shape[0] >= got['mask_index'].shape[0]  # (at least the default row of each pixel)
    assert np.isfinite(got['rows']).all()


def test_pmc_records_are_found_by_their_workload_keys():
    paths = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'pmc_*.json')))
    assert any(p.endswith('pmc_detect.json') for p in paths)
    keys = set()
    for p in paths:
        rec = json.load(open(p))
        for k in ('workload', 'hbm_bytes_per_launch', 'hbm_read_bytes', 'hbm_write_bytes', 'counters'):
            assert k in rec, (p, k)
        assert rec['hbm_bytes_per_launch'] == rec['hbm_read_bytes'] + rec['hbm_write_bytes']
        assert rec['workload'] not in keys, 'two records for one workload key'
        keys.add(rec['workload'])
        found, got = bench.pmc_record(rec['workload'])
        assert found == os.path.relpath(p, ROOT) and got == rec
    assert bench.pmc_record('no such workload') == (None, {})


def test_hardware_fp64_fraction_reproduces_from_the_committed_profiles():
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'pmc_detect.json')))
    c = rec['counters']
    rows = list(csv.DictReader(open(os.path.join(ROOT, 'profiles', 'r06', 'kernel_stats.csv'))))
    det = [r for r in rows if 'ccd_detect' in r['Name']]
    assert len(det) == 1
    ms = float(det[0]['AverageNs']) * 1e-6
    hw = bench.hardware_fp64(c, ms, 256)
    lane = 64 * (c['SQ_INSTS_VALU_ADD_F64'] + c['SQ_INSTS_VALU_MUL_F64'] + 2 * c['SQ_INSTS_VALU_FMA_F64']
                 + c['SQ_INSTS_VALU_TRANS_F64'])
    assert hw['lane_flops'] == lane
    assert abs(hw['frac'] - lane / (ms * 1e-3) / (bench.FP64_PEAK_TFLOPS * 1e12)) < 1e-12
    assert 0.0 < hw['frac'] < 1.0 and 0.0 < hw['valu_issue_model'] <= hw['valu_busy'] < 1.0
    assert bench.hardware_fp64({}, ms, 256) == {}
