"""numpy restatement of the transport encoding's bit-packed mode 2 (layout in include/ccdgpu.h):
a decoder (what ccd_decode_pack in ccd_pack.hip computes) and a slow canonical encoder (what
ccdgpu_encode_chips_flags with CCDGPU_ENC_PACK writes, byte for byte), shared by the CPU and GPU
tests of the packed encoding."""
import numpy as np

HDR = 128
ALIGN = 256


def up(x, a):
    return (x + a - 1) // a * a


def sections(buf):
    """[(offset, end)] of the chip sections and the chip pixel prefix"""
    buf = np.asarray(buf, dtype=np.uint8)
    nc = int(buf[:8].view(np.int64)[0])
    off = buf[8:8 * (nc + 2)].view(np.int64)
    pixo = buf[8 * (nc + 2):8 * (2 * nc + 3)].view(np.int64)
    return [(int(off[c]), int(off[c + 1])) for c in range(nc)], [int(p) for p in pixo]


def layout(sec):
    """offsets of a mode 2 section's parts: dict(koff, qa4, runs, codes, exc, end) and the header's
    n_pix, n_obs, kept, code_words, exc_total"""
    mode, n_pix, n_obs, n_pal = (int(v) for v in sec[:16].view(np.int32))
    assert mode == 2
    kept = int(sec[48:56].view(np.int64)[0])
    code_words, exc_total = (int(v) for v in sec[88:104].view(np.int64))
    rowb = (n_obs + 1) // 2
    koff = HDR
    qa4 = koff + up(4 * (n_pix + 1), 16)
    runs = qa4 + up(n_pix * rowb, 16)
    codes = runs + 112 * n_pix
    exc = codes + up(4 * (code_words + 1), 16)
    return dict(koff=koff, qa4=qa4, runs=runs, codes=codes, exc=exc, end=exc + 2 * exc_total, n_pix=n_pix,
                n_obs=n_obs, kept=kept, code_words=code_words, exc_total=exc_total, rowb=rowb)


RUN_DTYPE = np.dtype([('base', '<i2'), ('w', '<u2'), ('code_word', '<u4'), ('exc_off', '<u4'), ('n_exc', '<u4')])
assert RUN_DTYPE.itemsize == 16


def run_table(sec):
    """the run descriptors of a mode 2 section, a (n_pix, 7) view"""
    lay = layout(sec)
    return sec[lay['runs']:lay['codes']].view(RUN_DTYPE).reshape(lay['n_pix'], 7)


def widths(buf):
    """every run's width of every mode 2 section of a batch, flattened"""
    out = []
    for a, b in sections(buf)[0]:
        sec = np.asarray(buf, dtype=np.uint8)[a:b]
        if int(sec[:4].view(np.int32)[0]) == 2:
            out.append(run_table(sec)['w'].reshape(-1))
    return np.concatenate(out) if out else np.zeros(0, np.uint16)


def unpack_codes(words, k, w):
    """k codes of w bits from uint32 words: bit j of the run is bit j & 31 of word j >> 5"""
    if w == 0 or k == 0:
        return np.zeros(k, dtype=np.int64)
    bits = np.unpackbits(np.ascontiguousarray(words, dtype='<u4').view(np.uint8), bitorder='little')
    bits = bits[:k * w].reshape(k, w).astype(np.int64)
    return (bits << np.arange(w, dtype=np.int64)).sum(axis=1)


def decode(buf):
    """[(spectra [7][n_pix][n_obs], qa [n_pix][n_obs]), ...] of a batch of mode 0 and mode 2
    sections; dropped observations and every lane outside its run or exception list get -9999"""
    buf = np.asarray(buf, dtype=np.uint8)
    secs, pixo = sections(buf)
    out = []
    for c, (a, b) in enumerate(secs):
        sec = buf[a:b]
        mode, n_pix, n_obs, n_pal = (int(v) for v in sec[:16].view(np.int32))
        assert int(sec[72:80].view(np.int64)[0]) == pixo[c]
        plane = n_pix * n_obs
        if mode == 0:
            qa = sec[HDR:HDR + 2 * plane].view(np.uint16).reshape(n_pix, n_obs)
            s0 = HDR + up(2 * plane, 16)
            out.append((sec[s0:s0 + 14 * plane].view(np.int16).reshape(7, n_pix, n_obs).copy(), qa.copy()))
            continue
        assert mode == 2 and 1 <= n_pal <= 16
        assert int(sec[64:72].view(np.int64)[0]) == 0  # band_stride
        lay = layout(sec)
        pal = sec[16:48].view(np.uint16)
        drop = int(sec[80:84].view(np.uint32)[0])
        koff = sec[lay['koff']:lay['koff'] + 4 * (n_pix + 1)].view(np.uint32).astype(np.int64)
        q4 = sec[lay['qa4']:lay['qa4'] + n_pix * lay['rowb']].reshape(n_pix, lay['rowb'])
        nib = np.empty((n_pix, 2 * lay['rowb']), dtype=np.uint8)
        nib[:, 0::2] = q4 & 15
        nib[:, 1::2] = q4 >> 4
        qa = pal[nib[:, :n_obs]]
        keep = (qa & drop) == 0
        runs = run_table(sec)
        codes = sec[lay['codes']:lay['codes'] + 4 * (lay['code_words'] + 1)].view(np.uint32)
        assert codes[-1] == 0  # the pad word
        exc = sec[lay['exc']:lay['end']].view(np.int16)
        sp = np.full((7, n_pix, n_obs), -9999, dtype=np.int16)
        for p in range(n_pix):
            k = int(koff[p + 1] - koff[p])
            idx = np.flatnonzero(keep[p])[:k]
            for band in range(7):
                r = runs[p, band]
                w = int(r['w'])
                kk = len(idx)
                nw = (kk * w + 31) // 32
                cd = unpack_codes(codes[int(r['code_word']):int(r['code_word']) + nw], kk, w)
                v = (int(r['base']) + cd).astype(np.int64)
                if 1 <= w <= 15:
                    esc = cd == (1 << w) - 1
                    er = np.cumsum(esc) - 1
                    ok = esc & (er < int(r['n_exc']))
                    v[esc] = -9999
                    v[ok] = exc[int(r['exc_off']) + er[ok]]
                sp[band, p, idx] = ((v + 32768) % 65536 - 32768).astype(np.int16)
        out.append((sp, qa))
    return out


def choose_width(r):
    """the canonical width of a run of residuals r (int64, >= 0): the w of 0 .. 16 that minimises
    w k + 16 e(w), e(w) = count of r >= 2^w - 1 (w = 1 .. 15), e(16) = 0, w = 0 only when every r
    is 0; ties to the smallest w"""
    k = r.shape[0]
    if k == 0 or int(r.max()) == 0:
        return 0
    best, bw = None, None
    for w in range(1, 17):
        e = int((r >= (1 << w) - 1).sum()) if w < 16 else 0
        cost = w * k + 16 * e
        if best is None or cost < best:
            best, bw = cost, w
    return bw


def pack_run(v):
    """kept values of one (pixel, band) -> (base, w, uint32 code words, int16 exceptions)"""
    v = np.asarray(v, dtype=np.int64)
    k = v.shape[0]
    base = int(v.min()) if k else 0
    r = v - base
    w = choose_width(r)
    if w == 0:
        return base, 0, np.zeros(0, np.uint32), np.zeros(0, np.int16)
    if w < 16:
        esc = r >= (1 << w) - 1
        code = np.where(esc, (1 << w) - 1, r)
        ex = v[esc].astype(np.int16)
    else:
        code, ex = r, np.zeros(0, np.int16)
    bits = ((code[:, None] >> np.arange(w, dtype=np.int64)) & 1).astype(np.uint8).reshape(-1)
    nw = (k * w + 31) // 32
    bits = np.concatenate([bits, np.zeros(32 * nw - bits.shape[0], np.uint8)])
    return base, w, np.packbits(bits, bitorder='little').view('<u4').copy(), ex


def _raw_section(s, q, data_off, pix_base, drop_field):
    n_pix, n_obs = q.shape
    plane = n_pix * n_obs
    sec = np.zeros(HDR + up(2 * plane, 16) + 14 * plane, dtype=np.uint8)
    sec[:16].view(np.int32)[:] = [0, n_pix, n_obs, 0]
    sec[48:80].view(np.int64)[:] = [0, data_off, 0, pix_base]
    sec[80:84].view(np.uint32)[0] = drop_field
    sec[HDR:HDR + 2 * plane].view(np.uint16)[:] = q.reshape(-1)
    s0 = HDR + up(2 * plane, 16)
    sec[s0:].view(np.int16)[:] = s.reshape(-1)
    return sec


def encode(chips, drop=1, strict=1):
    """the bytes ccdgpu_encode_chips_flags(..., CCDGPU_ENC_PACK) writes for chips [(dates,
    spectra [7][n_pix][n_obs], qa [n_pix][n_obs]), ...]: mode 2 sections, and mode 0 for a chip with
    more than 16 QA words or a strict observation holding data"""
    nc = len(chips)
    tab = up(8 + 16 * (nc + 1), ALIGN)
    parts = []
    off, pix = [], []
    pos, pbase, dbase = tab, 0, 0
    for _, s, q in chips:
        s = np.ascontiguousarray(s, dtype=np.int16)
        q = np.ascontiguousarray(q, dtype=np.uint16)
        n_pix, n_obs = q.shape
        pal = np.unique(q)
        gone = (q & drop) != 0
        bad = bool(((s != -9999) & ((q & strict) != 0)[None]).any())
        if pal.shape[0] > 16:
            sec = _raw_section(s, q, dbase, pbase, 0)
        elif bad:
            sec = _raw_section(s, q, dbase, pbase, drop)
        else:
            keep = ~gone
            kc = keep.sum(axis=1).astype(np.int64)
            koff = np.concatenate([[0], np.cumsum(kc)])
            rowb = (n_obs + 1) // 2
            idx = np.searchsorted(pal, q).astype(np.uint8)
            nib = np.zeros((n_pix, 2 * rowb), dtype=np.uint8)
            nib[:, :n_obs] = idx
            q4 = nib[:, 0::2] | (nib[:, 1::2] << 4)
            runs = np.zeros((n_pix, 7), dtype=RUN_DTYPE)
            words, excs = [], []
            cw = ex = 0
            for p in range(n_pix):
                for band in range(7):
                    base, w, wd, e = pack_run(s[band, p, keep[p]])
                    runs[p, band] = (base, w, cw, ex, e.shape[0])
                    words.append(wd)
                    excs.append(e)
                    cw += wd.shape[0]
                    ex += e.shape[0]
            a_q = HDR + up(4 * (n_pix + 1), 16)
            a_r = a_q + up(n_pix * rowb, 16)
            a_c = a_r + 112 * n_pix
            a_e = a_c + up(4 * (cw + 1), 16)
            sec = np.zeros(a_e + 2 * ex, dtype=np.uint8)
            sec[:16].view(np.int32)[:] = [2, n_pix, n_obs, pal.shape[0]]
            sec[16:16 + 2 * pal.shape[0]].view(np.uint16)[:] = pal
            sec[48:80].view(np.int64)[:] = [int(koff[-1]), dbase, 0, pbase]
            sec[80:84].view(np.uint32)[0] = drop
            sec[88:104].view(np.int64)[:] = [cw, ex]
            sec[HDR:HDR + 4 * (n_pix + 1)].view(np.uint32)[:] = koff
            sec[a_q:a_q + n_pix * rowb] = q4.reshape(-1)
            sec[a_r:a_c] = runs.reshape(-1).view(np.uint8)
            if cw:
                sec[a_c:a_c + 4 * cw].view(np.uint32)[:] = np.concatenate(words)
            if ex:
                sec[a_e:].view(np.int16)[:] = np.concatenate(excs)
        off.append(pos)
        pix.append(pbase)
        parts.append(sec)
        pos += up(sec.shape[0], ALIGN)
        pbase += n_pix
        dbase += n_pix * n_obs
    off.append(pos)
    pix.append(pbase)
    buf = np.zeros(pos, dtype=np.uint8)
    buf[:8].view(np.int64)[0] = nc
    buf[8:8 * (nc + 2)].view(np.int64)[:] = off
    buf[8 * (nc + 2):8 * (2 * nc + 3)].view(np.int64)[:] = pix
    for o, sec in zip(off, parts):
        buf[o:o + sec.shape[0]] = sec
    return buf


# ---- hand-built chips that hit every edge of the layout
def _dates(n):
    return np.arange(n, dtype=np.int64) * 16 + 730000


CLEAR, CLOUD, FILL = 66, 66 | 32, 1  # QA words: clear, clear + cloud bit, fill


def edge_chip(n_obs, n_pix, seed):
    """A chip whose bands come out at w = 0, 1, 5, 12, 15 (with escapes) and 16 (band b of pixel p
    takes pattern (b + p) % 7, so every pixel count sees every width): negative values, a run
    spanning -32768 .. 32767, and -- the chip's last pixel, when it has more than one -- a pixel
    with nothing kept.  Pixel 0 keeps every observation (k = n_obs: with 64 observations w = 1
    and w = 16 end on a word boundary, w = 5, 12 and 15 straddle one; with 1 observation k = 1);
    the others drop a few as fill (-9999 in every band)."""
    rng = np.random.default_rng(seed)
    q = np.full((n_pix, n_obs), CLEAR, dtype=np.uint16)
    s = np.zeros((7, n_pix, n_obs), dtype=np.int16)
    for p in range(n_pix):
        for b in range(7):
            kind = (b + p) % 7
            if kind == 0:
                v = np.full(n_obs, -1234)
            elif kind == 1:
                v = np.full(n_obs, 7000)
                v[n_obs // 2] = 7001  # one value off the base: w = 1 with one escape (k > 16)
            elif kind == 2:
                v = -300 + rng.integers(0, 31, n_obs)
            elif kind == 3:
                v = 100 + rng.integers(0, 4095, n_obs)
            elif kind == 4:
                v = -20000 + rng.integers(0, 32767, n_obs)
                v[rng.random(n_obs) < 0.02] = 32000  # a few escapes
            elif kind == 5:
                v = rng.integers(-32768, 32768, n_obs)
                v[0] = -32768
                v[-1] = 32767
            else:
                v = 500 + rng.integers(0, 200, n_obs)
                v[rng.random(n_obs) < 0.1] = 20000  # escapes of a narrow run
            s[b, p] = v
    if n_pix > 1:
        q[-1, :] = FILL
        s[:, -1, :] = -9999
        for p in range(1, n_pix - 1):
            gone = rng.random(n_obs) < 0.2
            q[p, gone] = FILL
            s[:, p, gone] = -9999
    return _dates(n_obs), s, q


def escape_chip():
    """257 observations, 2 pixels: pixel 0 keeps all 257, band 0 is a narrow run (w small) with
    more than 64 escapes, among them positions 0, 63, 64 and k - 1; pixel 1 drops every third
    observation (cloud, data kept in place: only the 'unread' drop removes it)."""
    n = 257
    rng = np.random.default_rng(77)
    q = np.full((2, n), CLEAR, dtype=np.uint16)
    s = rng.integers(200, 230, size=(7, 2, n)).astype(np.int16)
    far = np.zeros(n, dtype=bool)
    far[[0, 63, 64, n - 1]] = True
    far[100:170] = True
    s[0, 0, far] = rng.integers(5000, 30000, int(far.sum())).astype(np.int16)  # (above the base: escapes)
    s[3, 1, ::5] = 25000
    q[1, ::3] = CLOUD
    return _dates(n), s, q


def edge_chips():
    """the edge shapes: n_obs in {1, 33, 64, 65, 257} x n_pix in {1, 5}, and the escape chip"""
    out = [edge_chip(n, p, 100 * n + p) for n in (1, 33, 64, 65, 257) for p in (1, 5)]
    out.append(escape_chip())
    return out


def plain_chip():
    """40 observations x 3 pixels, every band within 31 of its minimum: w <= 5 and no exceptions"""
    rng = np.random.default_rng(5)
    n = 40
    q = np.full((3, n), CLEAR, dtype=np.uint16)
    s = (1000 + rng.integers(0, 31, size=(7, 3, n))).astype(np.int16)
    return _dates(n), s, q


def check_chips():
    """the batch of the malformed-section checks: its last chip has no exceptions, so cutting its
    section after the last code word removes exactly the pad word"""
    return [edge_chip(65, 5, 1), escape_chip(), plain_chip()]


def malformed(enc):
    """[(name, EncodedBatch)]: copies of the packed batch ``enc`` (of check_chips()), each with one
    fault ccdgpu_encoded_check must find"""
    import copy
    secs, _ = sections(enc.buf[:enc.nbytes_encoded])
    nc = len(secs)
    out = []

    def variant(name, fn):
        b = copy.copy(enc)
        b.buf = enc.buf.copy()
        fn(b)
        out.append((name, b))

    def sec_of(b, c):
        return b.buf[secs[c][0]:secs[c][1]]

    def cut(b, nbytes):
        """the last section ends after nbytes"""
        end = secs[-1][0] + nbytes
        b.buf[8:8 * (nc + 2)].view(np.int64)[nc] = end
        b.nbytes_encoded = end

    def run_field(c, p, band, name, value):
        def fn(b):
            run_table(sec_of(b, c))[name][p, band] = value(run_table(sec_of(b, c))[name][p, band])
        return fn

    last = layout(sec_of(enc, nc - 1))
    assert last['exc_total'] == 0 and last['code_words'] > 8
    rt = run_table(sec_of(enc, 1))
    assert int(rt['n_exc'][0, 0]) > 64
    variant('w = 17', run_field(0, 1, 2, 'w', lambda v: 17))
    variant('code_word off by one', run_field(0, 2, 0, 'code_word', lambda v: v + 1))
    # chip 1's last run claims one exception more: exc_off + n_exc passes exc_total
    variant('exceptions past exc_total', run_field(1, 1, 6, 'n_exc', lambda v: v + 1))
    variant('wrong code_words', lambda b: sec_of(b, 0)[88:96].view(np.int64).__setitem__(0, layout(sec_of(enc, 0))['code_words'] + 1))
    variant('truncated inside the codes', lambda b: cut(b, last['codes'] + 16))
    variant('no pad word', lambda b: cut(b, last['codes'] + 4 * last['code_words']))
    return out


def exact_end(enc):
    """a copy of ``enc`` whose last section ends right behind its (16-byte padded) codes part:
    still a valid batch"""
    import copy
    secs, _ = sections(enc.buf[:enc.nbytes_encoded])
    nc = len(secs)
    last = layout(enc.buf[secs[-1][0]:secs[-1][1]])
    b = copy.copy(enc)
    b.buf = enc.buf.copy()
    end = secs[-1][0] + last['end']
    b.buf[8:8 * (nc + 2)].view(np.int64)[nc] = end
    b.nbytes_encoded = end
    return b
