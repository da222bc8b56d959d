"""Bit-packed band runs of the transport encoding (mode 2 sections: ccdgpu_encode_chips_flags with
CCDGPU_ENC_PACK, include/ccdgpu.h): the C encoder's bytes equal a slow numpy encoder's and decode
-- with a numpy restatement of the device decoder -- to the inputs, for every edge of the layout;
the bytes do not depend on the thread count or on the scalar / vector path; the packed batches are
smaller than mode 1's and stay within their bound; ccdgpu_encoded_check refuses malformed
sections.  CPU only (no device)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'lcmap-firebird_amd'))

ccdgpu = pytest.importorskip('ccdgpu')
from ccdgpu import synth  # noqa: E402

import encode_util  # noqa: E402
import pack_util  # noqa: E402


def encode(chips, threads=3, drop=1, strict=1, pack=True):
    e = ccdgpu.EncodedBatch.encode(chips, threads=threads, pinned=False, drop_bits=drop, strict_bits=strict, pack=pack)
    return e, e.buf[:e.nbytes_encoded]


def check_roundtrip(chips, drop=1, strict=1):
    """C bytes == numpy bytes; the numpy decoder gives the inputs back (-9999 where dropped)"""
    e, buf = encode(chips, drop=drop, strict=strict)
    e.check()
    ref = pack_util.encode(chips, drop, strict)
    assert buf.shape == ref.shape and np.array_equal(buf, ref)
    for (d, s, q), (ds, dq) in zip(chips, pack_util.decode(buf)):
        np.testing.assert_array_equal(dq, q)
        gone = (q & drop) != 0
        np.testing.assert_array_equal(ds[:, ~gone], s[:, ~gone])
        assert (ds[:, gone] == -9999).all()
    return e, buf


@pytest.fixture(scope='module')
def edge():
    return pack_util.edge_chips()


def test_edge_chips_roundtrip_and_match_the_numpy_encoder(edge):
    e, buf = check_roundtrip(edge)
    assert e.chip_modes() == [2] * len(edge)
    assert {0, 1, 5, 12, 15, 16} <= set(pack_util.widths(buf).tolist())
    secs, _ = pack_util.sections(buf)
    by_shape = {}
    for (d, s, q), (a, b) in zip(edge, secs):
        by_shape[(q.shape[1], q.shape[0], len(by_shape))] = (s, q, buf[a:b])
    for (n_obs, n_pix, _), (s, q, sec) in by_shape.items():
        rt = pack_util.run_table(sec)
        koff = sec[128:128 + 4 * (n_pix + 1)].view(np.uint32)
        if n_pix == 5:  # the last pixel keeps nothing: base 0, w 0, no words
            assert koff[5] == koff[4]
            assert (rt['w'][4] == 0).all() and (rt['base'][4] == 0).all() and (rt['n_exc'][4] == 0).all()
        if n_obs == 1 and n_pix == 1:  # k = 1: the value is the base
            assert koff[1] == 1 and (rt['w'][0] == 0).all()
            np.testing.assert_array_equal(rt['base'][0], s[:, 0, 0])
        ws = set(int(w) for w in rt['w'][0])
        if n_obs == 64:  # pixel 0 keeps 64 values: every run's last code ends exactly on a word boundary,
            assert koff[1] == 64 and 16 in ws  # and codes of a width that does not divide 32 straddle words inside
            assert any(32 % w for w in ws if w)
        if n_obs == 65:  # 65 values: the last code of a run ends inside a word
            assert koff[1] == 65 and any((65 * w) % 32 for w in ws if w)
    # a run spanning -32768 .. 32767 sits at w = 16 with base -32768
    full = [(int(r['base']), int(r['w'])) for (a, b) in secs for r in pack_util.run_table(buf[a:b]).reshape(-1)]
    assert (-32768, 16) in full
    assert any(b < 0 for b, _ in full)


def test_run_with_more_than_64_escapes(edge):
    e, buf = encode([pack_util.escape_chip()])
    (a, b), = pack_util.sections(buf)[0]
    rt = pack_util.run_table(buf[a:b])
    r = rt[0, 0]
    assert 1 <= int(r['w']) <= 15 and int(r['n_exc']) > 64
    d, s, q = pack_util.escape_chip()
    lay = pack_util.layout(buf[a:b])
    k = 257
    codes = pack_util.unpack_codes(buf[a:b][lay['codes']:lay['codes'] + 4 * lay['code_words']].view(np.uint32)[
        int(r['code_word']):int(r['code_word']) + (k * int(r['w']) + 31) // 32], k, int(r['w']))
    esc = codes == (1 << int(r['w'])) - 1
    assert esc[[0, 63, 64, k - 1]].all() and int(esc.sum()) == int(r['n_exc'])
    check_roundtrip([pack_util.escape_chip()])
    drop, strict = ccdgpu.unread_drop_bits(None)
    check_roundtrip([pack_util.escape_chip()], drop, strict)


def _child(code):
    outs = {}
    for scalar in ('0', '1'):
        env = dict(os.environ, CCDGPU_ENCODE_SCALAR=scalar)
        outs[scalar] = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, check=True).stdout
    return outs


def test_bytes_do_not_depend_on_threads_or_the_vector_path(edge):
    chips = edge + [synth.chip(synth.config(3), 0, 0, 97)]
    _, b1 = encode(chips, threads=1)
    _, b4 = encode(chips, threads=4)
    assert np.array_equal(b1, b4)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import ccdgpu, pack_util; "
            "from ccdgpu import synth; chips = pack_util.edge_chips() + [synth.chip(synth.config(3), 0, 0, 97)]; "
            "e = ccdgpu.EncodedBatch.encode(chips, threads=4, pinned=False, pack=True); "
            "sys.stdout.buffer.write(bytes([int(ccdgpu.encode_vector_path())]) + e.buf[:e.nbytes_encoded].tobytes())"
            % (os.path.join(ROOT, 'lcmap-firebird_amd'), HERE))
    outs = _child(code)
    assert outs['1'][0] == 0
    assert outs['1'][1:] == b1.tobytes()  # the scalar path against this process's bytes
    if outs['0'][0] == 0:
        pytest.skip('no AVX-512 VBMI2 on this CPU: only the scalar encoder ran')
    assert outs['0'][1:] == outs['1'][1:]


@pytest.mark.parametrize('which', [2, 3, 4, 5])
def test_synthetic_chips_roundtrip(which):
    cfg = synth.config(which)
    chips = [synth.chip(cfg, 7, 0, 40), synth.chip(cfg, 8, 0, 23)]
    check_roundtrip(chips)
    drop, strict = ccdgpu.unread_drop_bits(None)
    check_roundtrip(chips, drop, strict)


def test_packed_batches_are_smaller_than_mode_1():
    """C3 chips 0 and 1, 200 pixels: packed / mode 1 bytes below 0.80 ('unread'; the numpy model
    gives about 0.72) and below 0.85 ('lossless'; about 0.79).  The numpy encoder meets both caps
    at this shape, so they stand as set."""
    cfg = synth.config(3)
    chips = [synth.chip(cfg, c, 0, 200) for c in (0, 1)]
    drop, strict = ccdgpu.unread_drop_bits(None)
    for name, (dr, st), cap in (('unread', (drop, strict), 0.80), ('lossless', (1, 1), 0.85)):
        m1, _ = encode(chips, threads=4, drop=dr, strict=st, pack=False)
        ref = pack_util.encode(chips, dr, st).shape[0]
        e, _ = encode(chips, threads=4, drop=dr, strict=st)
        assert m1.chip_modes() == [1, 1] and e.chip_modes() == [2, 2]
        print('%s: mode 1 %d B, packed %d B (numpy %d B), ratio %.4f' % (name, m1.nbytes_encoded, e.nbytes_encoded, ref,
                                                                        e.nbytes_encoded / m1.nbytes_encoded))
        assert ref < cap * m1.nbytes_encoded, name  # the reference itself
        assert e.nbytes_encoded == ref
        assert e.nbytes_encoded < cap * m1.nbytes_encoded, name


def test_full_range_data_stays_within_the_bound():
    rng = np.random.default_rng(21)
    chips = []
    for n_pix, n_obs in ((7, 33), (3, 257), (1, 1), (40, 64)):
        q = np.full((n_pix, n_obs), 66, dtype=np.uint16)
        s = rng.integers(-32768, 32768, size=(7, n_pix, n_obs)).astype(np.int16)
        chips.append((np.arange(n_obs, dtype=np.int64), s, q))
    e, buf = check_roundtrip(chips)
    w = pack_util.widths(buf)
    big = np.concatenate([pack_util.run_table(buf[a:b])['w'].reshape(-1) for (a, b) in pack_util.sections(buf)[0]
                          if buf[a + 8:a + 12].view(np.int32)[0] > 2])  # chips with more than 2 observations
    assert (big == 16).all() and w.max() == 16
    np_ = np.array([c[2].shape[0] for c in chips], dtype=np.int32)
    no = np.array([c[2].shape[1] for c in chips], dtype=np.int32)
    bound = int(ccdgpu.lib().ccdgpu_encoded_bound_flags(len(chips), np_.ctypes.data, no.ctypes.data, 1))
    plain = int(ccdgpu.lib().ccdgpu_encoded_bound(len(chips), np_.ctypes.data, no.ctypes.data))
    assert e.nbytes_encoded <= bound == e.bound
    assert int(ccdgpu.lib().ccdgpu_encoded_bound_flags(len(chips), np_.ctypes.data, no.ctypes.data, 0)) == plain
    # one chip at a time too (the bound holds per section)
    for c in chips:
        e1, _ = encode([c])
        assert e1.nbytes_encoded <= e1.bound


def test_flags_zero_is_the_plain_encoding():
    cfg = synth.config(3)
    chips = [synth.chip(cfg, 0, 0, 60)] + pack_util.edge_chips()[:4]
    e0, b0 = encode(chips, pack=False)
    assert set(e0.chip_modes()) <= {0, 1} and 1 in e0.chip_modes()
    for (d, s, q), (ds, dq) in zip(chips, encode_util.decode(b0)):
        np.testing.assert_array_equal(ds, s)
        np.testing.assert_array_equal(dq, q)
    # the _flags entry point with flags = 0 writes the same bytes as the plain one
    import ctypes
    L = ccdgpu.lib()
    sp = (ctypes.c_void_p * len(chips))(*[np.ascontiguousarray(c[1]).ctypes.data for c in chips])
    qp = (ctypes.c_void_p * len(chips))(*[np.ascontiguousarray(c[2]).ctypes.data for c in chips])
    out = np.zeros(e0.bound, dtype=np.uint8)
    n = L.ccdgpu_encode_chips_flags(len(chips), e0.n_pix.ctypes.data, e0.n_obs.ctypes.data,
                                    ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(qp, ctypes.c_void_p), out.ctypes.data,
                                    out.size, 2, 1, 1, 0)
    assert n == e0.nbytes_encoded and np.array_equal(out[:n], b0)
    assert L.ccdgpu_encode_chips_flags(len(chips), e0.n_pix.ctypes.data, e0.n_obs.ctypes.data,
                                       ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(qp, ctypes.c_void_p),
                                       out.ctypes.data, out.size, 2, 1, 1, 2) < 0  # an unknown flag


def test_raw_fallbacks_in_a_packed_batch():
    rng = np.random.default_rng(5)
    n = 33
    d = np.arange(n, dtype=np.int64) * 16 + 730000
    q_many = rng.integers(2, 4000, size=(5, n)).astype(np.uint16) & ~np.uint16(1)
    s_many = rng.integers(-100, 10000, size=(7, 5, n)).astype(np.int16)
    q_bad = np.full((3, n), 66, dtype=np.uint16)
    q_bad[1, 4] = 1
    s_bad = rng.integers(0, 5000, size=(7, 3, n)).astype(np.int16)
    s_bad[:, 1, 4] = -9999
    s_bad[3, 1, 4] = 17
    chips = [(d, s_many, q_many), pack_util.edge_chip(33, 5, 3), (d, s_bad, q_bad)]
    e, buf = encode(chips)
    assert e.chip_modes() == [0, 2, 0]
    assert np.array_equal(buf, pack_util.encode(chips))
    for (d, s, q), (ds, dq) in zip(chips, pack_util.decode(buf)):
        np.testing.assert_array_equal(ds, s)
        np.testing.assert_array_equal(dq, q)


def test_check_rejects_malformed_packed_sections():
    e, _ = encode(pack_util.check_chips(), threads=2)
    assert e.chip_modes() == [2, 2, 2]
    e.check()
    pack_util.exact_end(e).check()  # a section that ends right behind its pad word is whole
    want = {'w = 17': 'width above 16', 'code_word off by one': 'prefix sums',
            'exceptions past exc_total': 'totals', 'wrong code_words': 'totals',
            'truncated inside the codes': 'truncated', 'no pad word': 'truncated'}
    bad = pack_util.malformed(e)
    assert [n for n, _ in bad] == list(want)
    for name, b in bad:
        with pytest.raises(ccdgpu.CcdGpuError, match='encoded batch') as ei:
            b.check()
        assert want[name] in str(ei.value), (name, str(ei.value))
    # modes 1 and 2 never share a batch: chip 0 from a mode 1 batch of the same chips, chip 1 packed
    cs = pack_util.check_chips()[:2]
    e1, b1 = encode(cs, pack=False)
    e2, b2 = encode(cs)
    (a0, a1), _ = pack_util.sections(b1)[0]
    _, (c0, c1) = pack_util.sections(b2)[0]
    import copy
    mixed = copy.copy(e2)
    mixed.buf = np.zeros(a1 + (c1 - c0), dtype=np.uint8)
    mixed.buf[:a1] = b1[:a1]
    mixed.buf[a1:] = b2[c0:c1]
    mixed.buf[8:32].view(np.int64)[:] = [a0, a1, a1 + c1 - c0]
    mixed.nbytes_encoded = mixed.buf.size
    with pytest.raises(ccdgpu.CcdGpuError, match='mode 1 and mode 2'):
        mixed.check()


def test_encoding_source_passes_pack_through():
    """ccdc.runner.EncodingSource(pack=True) hands out packed batches (sized by the packed bound,
    from reused storage too) that decode to the inputs; the default stays mode 1"""
    from ccdc import runner
    chips = [synth.chip(synth.config(3), 0, 0, 30), synth.chip(synth.config(4), 1, 0, 20)]

    class Src(object):
        has_views = True

        def views(self, positions):
            return [chips[p] for p in positions]

    plain = runner.EncodingSource(Src(), threads=2, pinned=False, drop='lossless')
    packed = runner.EncodingSource(Src(), threads=2, pinned=False, drop='lossless', pack=True)
    assert plain([0, 1]).chip_modes() == [1, 1]
    for _ in range(2):  # the second batch comes from the released storage
        b = packed([0, 1])
        assert b.chip_modes() == [2, 2]
        b.check()
        for (d, s, q), (ds, dq) in zip(chips, pack_util.decode(b.buf[:b.nbytes_encoded])):
            np.testing.assert_array_equal(ds, s)
            np.testing.assert_array_equal(dq, q)
        packed.release(b)
    assert packed.bytes_sent < plain.bytes_sent * 2 and packed.bytes_raw == 2 * plain.bytes_raw


def test_native_round_trip_under_sanitizers(tmp_path):
    """tests/native/pack_check.c: the encoder and a plain-C decoder in one stand-alone program,
    about 200 random small chips at random widths and thread counts, built with
    -fsanitize=address,undefined -- round trip, and nothing written past the returned bytes."""
    exe = str(tmp_path / 'pack_check')
    cmd = ['gcc', '-O1', '-g', '-fopenmp', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-o', exe, os.path.join(HERE, 'native', 'pack_check.c')]
    probe = subprocess.run(['gcc', '-fsanitize=address,undefined', '-x', 'c', '-o', str(tmp_path / 'probe'), '-'],
                           input='int main(void){return 0;}', capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip('the compiler cannot link -fsanitize=address,undefined')
    subprocess.run(cmd, check=True)
    for scalar in ('0', '1'):
        out = subprocess.run([exe], env=dict(os.environ, CCDGPU_ENCODE_SCALAR=scalar, ASAN_OPTIONS='detect_leaks=1'),
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith('ok'), out.stdout


def test_native_host_checks_under_sanitizers(tmp_path):
    """tests/native/host_checks.cpp: the host API's validators (csrc/ccdgpu_checks.cpp, no HIP in
    it) and the encoder in one stand-alone program built with -fsanitize=address,undefined --
    ccdgpu_encoded_check accepts the encoder's batches (modes 0, 1 and 2) from a heap block of
    exactly their size and refuses every strict prefix from a block of exactly its size; the
    forest checks and forest_build on a hand-made forest; make_shape and check_params."""
    csrc = os.path.join(ROOT, 'lcmap-firebird_amd', 'csrc')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    inc = ['-I', os.path.join(ROOT, 'include')]
    probe = subprocess.run(['gcc', '-fsanitize=address,undefined', '-x', 'c', '-o', str(tmp_path / 'probe'), '-'],
                           input='int main(void){return 0;}', capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip('the compiler cannot link -fsanitize=address,undefined')
    enc_o, exe = str(tmp_path / 'ccd_encode.o'), str(tmp_path / 'host_checks')
    subprocess.run(['gcc', '-O1', '-g', '-fopenmp', '-c'] + san + inc + ['-o', enc_o, os.path.join(csrc, 'ccd_encode.c')],
                   check=True)
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fopenmp'] + san + inc +
                   ['-o', exe, os.path.join(HERE, 'native', 'host_checks.cpp'), os.path.join(csrc, 'ccdgpu_checks.cpp'), enc_o],
                   check=True)
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith('ok'), out.stdout
