"""Bit-packed band runs on the GPU (mode 2 sections of the transport encoding, decoded by
ccd_decode_pack on the copy stream): a packed batch stages exactly the inputs the raw upload
stages -- every edge of the layout, raw-fallback chips in the same batch -- and detects the same;
malformed sections are refused before the upload; a mode 1 batch after a packed one still decodes."""
import numpy as np
import pytest

import pack_util

pytestmark = pytest.mark.gpu


def staged(ctx, slot, batch, run=True):
    ctx.stage_slot_chips(slot, batch)
    ctx.run_slot(slot)
    s, q = ctx.staged_inputs()
    return s, q, [ctx.fetch(c) for c in range(batch.n_chips)]


def same_results(r0, r1):
    for a, b in zip(r0, r1):
        assert a.segments.tobytes() == b.segments.tobytes()
        assert np.array_equal(a.procedure, b.procedure) and np.array_equal(a.mask, b.mask)


def test_edge_chips_and_a_raw_fallback_stage_the_raw_inputs():
    import ccdgpu
    cs = pack_util.edge_chips()
    # a chip with more than 16 distinct QA words: sent raw (mode 0) inside the packed batch
    rng = np.random.default_rng(9)
    n = 70
    q_many = (rng.integers(1, 200, size=(6, n)) * 2).astype(np.uint16)
    s_many = rng.integers(-2000, 12000, size=(7, 6, n)).astype(np.int16)
    cs.insert(3, (np.arange(n, dtype=np.int64) * 8 + 730000, s_many, q_many))
    raw = ccdgpu.ChipBatch.from_chips(cs, pinned=True)
    enc = ccdgpu.EncodedBatch.encode(cs, threads=4, pack=True)
    modes = enc.chip_modes()
    assert modes[3] == 0 and modes[:3] + modes[4:] == [2] * (len(cs) - 1)
    assert {0, 1, 5, 12, 15, 16} <= set(pack_util.widths(enc.buf[:enc.nbytes_encoded]).tolist())
    ctx = ccdgpu.Context(0)
    try:
        ctx.stage_slot_encoded(1, enc)
        ctx.run_slot(1)
        s1, q1 = ctx.staged_inputs()
    finally:
        ctx.close()
    np.testing.assert_array_equal(q1, np.asarray(raw.qa))
    np.testing.assert_array_equal(s1, np.asarray(raw.spectra))


def test_synthetic_chips_stage_and_detect_the_same():
    import ccdgpu
    from ccdgpu import synth
    cs = [synth.chip(synth.config(3), 0, 0, 300), synth.chip(synth.config(4), 2, 0, 150),
          synth.chip(synth.config(5), 6, 0, 100)]
    raw = ccdgpu.ChipBatch.from_chips(cs, pinned=True)
    enc = ccdgpu.EncodedBatch.encode(cs, threads=4, pack=True)
    assert enc.chip_modes() == [2, 2, 2]
    assert enc.nbytes_encoded < 0.75 * (raw.spectra.nbytes + raw.qa.nbytes)
    ctx = ccdgpu.Context(0)
    try:
        s0, q0, r0 = staged(ctx, 0, raw)
        s1, q1, r1 = staged(ctx, 1, enc)
    finally:
        ctx.close()
    np.testing.assert_array_equal(q1, q0)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(s1, np.asarray(raw.spectra))
    same_results(r0, r1)


def test_unread_packed_stages_what_unread_mode_1_stages():
    import ccdgpu
    from ccdgpu import synth
    cs = [synth.chip(synth.config(3), 5, 0, 200), synth.chip(synth.config(2), 8, 0, 100), pack_util.escape_chip()]
    drop, strict = ccdgpu.unread_drop_bits(None)
    m1 = ccdgpu.EncodedBatch.encode(cs, threads=4, drop_bits=drop, strict_bits=strict)
    m2 = ccdgpu.EncodedBatch.encode(cs, threads=4, drop_bits=drop, strict_bits=strict, pack=True)
    assert m1.chip_modes() == [1, 1, 1] and m2.chip_modes() == [2, 2, 2]
    assert m2.nbytes_encoded < m1.nbytes_encoded
    ctx = ccdgpu.Context(0)
    try:
        s1, q1, r1 = staged(ctx, 0, m1)
        s2, q2, r2 = staged(ctx, 1, m2)
    finally:
        ctx.close()
    np.testing.assert_array_equal(q2, q1)
    np.testing.assert_array_equal(s2, s1)
    assert ((np.asarray(q1) & drop) != 0).any()  # (observations whose bands both encodings dropped)
    same_results(r1, r2)


def test_malformed_packed_batches_are_refused_and_a_mode_1_batch_follows():
    """every malformed batch of the CPU test is refused by stage_slot_encoded (before anything is
    uploaded); the intact packed batch then stages and runs; a mode 1 batch of the same chips staged
    after it in the same context decodes to the same inputs"""
    import ccdgpu
    cs = pack_util.check_chips()
    enc = ccdgpu.EncodedBatch.encode(cs, threads=2, pack=True)
    assert enc.chip_modes() == [2, 2, 2]
    raw = ccdgpu.ChipBatch.from_chips(cs, pinned=True)
    m1 = ccdgpu.EncodedBatch.encode(cs, threads=2)
    assert m1.chip_modes() == [1, 1, 1]
    ctx = ccdgpu.Context(0)
    try:
        for name, bad in pack_util.malformed(enc):
            with pytest.raises(ccdgpu.CcdGpuError) as ei:
                ctx.stage_slot_encoded(0, bad)
            assert 'encoded batch' in str(ei.value), name
        s2, q2, r2 = staged(ctx, 0, enc)
        s1, q1, r1 = staged(ctx, 1, m1)
    finally:
        ctx.close()
    np.testing.assert_array_equal(q2, np.asarray(raw.qa))
    np.testing.assert_array_equal(s2, np.asarray(raw.spectra))
    np.testing.assert_array_equal(q1, q2)
    np.testing.assert_array_equal(s1, s2)
    same_results(r1, r2)


def test_tile_runner_with_encode_pack_gives_the_same_rows():
    """ccdc.runner.changedetection(encode_pack=True): the same per-chip row digests as the default
    (mode 1) upload, for both drop settings, and fewer bytes sent"""
    import json
    import os
    import ccdgpu
    from ccdc import runner
    from ccdgpu import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'tests', 'golden', 'chipmunk', 'tile_response.json')) as f:
        tile = json.load(f)
    cache = {}

    def source(pos):
        for p in pos:
            if p not in cache:
                cache[p] = synth.chip(synth.config(5 if p % 3 == 2 else 3), p, 0, 120)
        return ccdgpu.ChipBatch.from_chips([cache[p] for p in pos], pinned=True)

    def run(encode, pack):
        res = runner.changedetection(tile, source, device=0, contexts=2, batch_chips=2, number=5,
                                     sink=runner.SummarySink(), encode=encode, encode_pack=pack)
        st = res['ranks'][0]
        return [c['digest'] for c in res['chips']], st['upload_bytes_sent'], st['upload_bytes_raw']

    for encode in (True, 'lossless'):
        d1, sent1, raw1 = run(encode, False)
        d2, sent2, raw2 = run(encode, True)
        assert d1 == d2 and raw1 == raw2
        assert sent2 < 0.9 * sent1
