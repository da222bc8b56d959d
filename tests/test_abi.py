"""C-ABI checks that need no GPU: the libraries load, export every symbol the headers declare,
and the struct layouts agree between include/ccdgpu.h and the ctypes mirror."""
import ctypes
import os
import re

import pytest

import ccdgpu
from ccdgpu import abi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    txt = open(os.path.join(ROOT, 'include', header)).read()
    return sorted(set(re.findall(r'\b(ccd(?:gpu|synth)_[a-z_]+)\s*\(', txt)))


def prototypes(header):
    """[(name, return type, [argument, ...])] of the header's functions, in its order: plain
    ``type name(args);`` at the start of a line, possibly over several lines, ``(void)`` for none."""
    txt = open(os.path.join(ROOT, 'include', header)).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    txt = re.sub(r'^[ \t]*#.*$', ' ', txt, flags=re.M)
    out = []
    for ret, name, args in re.findall(r'^([\w \*]+?)\b(ccd(?:gpu|synth)_\w+)\s*\(([^()]*)\)\s*;', txt, flags=re.M):
        args = [' '.join(a.split()) for a in args.split(',')]
        out.append((name, ' '.join(ret.split()), [] if args == ['void'] else args))
    return out


RESTYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t,
            'const char *': ctypes.c_char_p, 'void': None}
# C scalar type -> (bytes, 'i' signed / 'u' unsigned / 'f' floating)
SCALARS = {'int': (ctypes.sizeof(ctypes.c_int), 'i'), 'int32_t': (4, 'i'), 'uint16_t': (2, 'u'), 'uint32_t': (4, 'u'),
           'int64_t': (8, 'i'), 'size_t': (ctypes.sizeof(ctypes.c_size_t), 'u'), 'double': (8, 'f')}


def is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)


def scalar_kind(t):
    if t in (ctypes.c_float, ctypes.c_double):
        return ctypes.sizeof(t), 'f'
    return ctypes.sizeof(t), 'i' if t(-1).value < 0 else 'u'


@pytest.mark.parametrize('header,signatures', [('ccdgpu.h', abi.SIGNATURES), ('ccdsynth.h', synth.SIGNATURES)])
def test_signature_table_matches_the_header(header, signatures):
    """Every prototype of the header against the table the loader declares from: the same names in the
    same order, the argument count, the return type, and per argument pointer against pointer or a
    scalar of the C type's width and signedness."""
    protos = prototypes(header)
    assert [p[0] for p in protos] == list(signatures)
    assert sorted(p[0] for p in protos) == declared(header)  # (the parser missed no declaration)
    for name, ret, args in protos:
        restype, argtypes = signatures[name]
        assert restype is RESTYPES[ret], (name, ret, restype)
        assert len(argtypes) == len(args), (name, args, argtypes)
        for a, t in zip(args, argtypes):
            if '*' in a:
                assert is_pointer(t), (name, a, t)
            else:
                ctype = ' '.join(w for w in a.split()[:-1] if w != 'const')
                assert not is_pointer(t) and scalar_kind(t) == SCALARS[ctype], (name, a, t)


class _Symbol(object):
    restype = argtypes = 'unset'


def test_declare_skips_a_symbol_the_library_lacks():
    """A library built before a symbol (an A/B run against an older one) still loads: every symbol it
    has is declared from the table, the one it lacks is left for ctypes to name when called."""
    missing = 'ccdgpu_chip_row_count'

    class Lib(object):
        pass
    L = Lib()
    for name in abi.SIGNATURES:
        if name != missing:
            setattr(L, name, _Symbol())
    assert ccdgpu._declare(L) is L
    assert not hasattr(L, missing)
    for name, (restype, argtypes) in abi.SIGNATURES.items():
        if name != missing:
            assert getattr(L, name).restype is restype and getattr(L, name).argtypes == list(argtypes), name


def test_libccdgpu_exports_every_declared_symbol():
    L = ccdgpu.lib()
    names = declared('ccdgpu.h')
    assert 'ccdgpu_detect_batch' in names
    for n in names:
        assert hasattr(L, n), n
    assert set(names) == set(ccdgpu.EXPORTS)


def test_libccdsynth_exports_every_declared_symbol():
    L = synth.lib()
    for n in declared('ccdsynth.h'):
        assert hasattr(L, n), n


def test_struct_sizes_and_defaults():
    assert ctypes.sizeof(abi.Segment) == 4 * 6 + 8 + 8 * (7 * 3 + 49)
    p = ccdgpu.default_params()  # host-only entry point, no device needed
    q = abi.default_params()
    for name, _ in abi.Params._fields_:
        assert getattr(p, name) == getattr(q, name), name
    assert 'gfx950' in ccdgpu.version()


def test_params_from_pyccd_dict():
    p = abi.params_from_dict({'PEEK_SIZE': 8, 'DETECTION_BANDS': [1, 3], 'CURVE_QA': {'START': 15},
                              'ADAPTIVE_PEEK': False})
    assert p.peek_size == 8 and p.detection_bands == 0b1010 and p.curve_qa_start == 15
    assert p.adaptive_peek == 0
    with pytest.raises(KeyError):
        abi.params_from_dict({'NOT_A_PARAM': 1})


def test_init_without_gpu_fails_loudly():
    """No CPU fallback: on a host with no gfx950 device the context refuses to come up."""
    if ccdgpu.device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(ccdgpu.CcdGpuError):
        ccdgpu.Context(0)
    with pytest.raises(ccdgpu.CcdGpuError):
        ccdgpu.Context(0, copy_cus=8)


def test_init_rejects_a_negative_cu_reservation():
    with pytest.raises(ccdgpu.CcdGpuError, match='copy_cus'):
        ccdgpu.Context(0, copy_cus=-1)


def test_header_constants_match_the_binding():
    txt = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    assert int(re.search(r'#define CCDGPU_UPLOAD_SLOTS (\d+)', txt).group(1)) == ccdgpu.UPLOAD_SLOTS


def test_stats_struct_carries_the_pool_fields():
    names = [n for n, _ in abi.Stats._fields_]
    assert names[-4:] == ['pool_reruns', 'pool_cap', 'wave_slots', 'n_cu']
    txt = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    body = txt[txt.index('typedef struct ccdgpu_stats'):txt.index('} ccdgpu_stats;')]
    assert re.findall(r'\b(\w+);', body) == names


class _FakeLib(object):
    """ccdgpu_run_slot_end_rows of a finished batch: return code ``rc``, ``rows`` rows"""

    def __init__(self, rc, rows, msg):
        self.rc, self.rows, self.msg = rc, rows, msg

    def ccdgpu_run_slot_end_rows(self, ctx, secs, nr):
        nr._obj.value = self.rows
        return self.rc

    def ccdgpu_last_error(self):
        return self.msg.encode()


@pytest.mark.parametrize('rc,msg,qa', [(abi.E_QA, 'unsupported bit-packed QA value (pixel 7)', True),
                                       (abi.E_OVERFLOW, 'run_slot_end_rows: 900 rows, the buffer holds 264', False)])
def test_run_slot_end_rows_fetches_short_rows_and_keeps_the_qa_error(monkeypatch, rc, msg, qa):
    """Context.run_slot_end_rows (ccdgpu/__init__.py) after a chain whose rows did not fit the copy:
    the rows are fetched into grown buffers whether the library says CCDGPU_EOVERFLOW or -- the
    batch also holding an unsupported QA value -- CCDGPU_EQA with the row count set; qa_error
    follows the return code (the tile runner raises on it)."""
    ctx = object.__new__(ccdgpu.Context)
    ctx.qa_error = False
    ctx._ctx = None
    bufs = ccdgpu.RowsBuffers(pinned=False, rows_per_pixel=0.5)
    ctx._rows_req = ([0], [0], bufs, 100, 400, 13, 264)
    ctx._pending_slot = 0
    ctx._slots = {0: ccdgpu._Staged(object())}
    fetched = []
    ctx.fetch_batch_rows_into = lambda cx, cy, b, w: fetched.append(b) or ('rows',)
    monkeypatch.setattr(ccdgpu, 'lib', lambda: _FakeLib(rc, 900, msg))
    out = ctx.run_slot_end_rows()
    assert out == ('rows',) and fetched == [bufs]
    assert ctx.qa_error is qa
    assert bufs.rows_per_pixel >= 1.25 * 900 / 400


def test_rows_buffers_learn_from_an_overflow():
    """RowsBuffers.learn with the numbers of the chain above: 900 rows of 400 pixels against a copy of
    264 say fetch, raise the room to at least 1.25 x the rate and the copy to 1.25 x the highest rate
    seen, within the room."""
    bufs = ccdgpu.RowsBuffers(pinned=False, rows_per_pixel=0.5)
    assert bufs.learn(900, 400, 264) is True
    assert bufs.max_rate == 900 / 400
    assert bufs.rows_per_pixel >= 1.25 * 900 / 400
    assert bufs.copy_per_pixel == min(bufs.rows_per_pixel, 1.25 * 900 / 400)


def test_rows_buffers_learn_without_an_overflow():
    """Rows that fit the copy move only max_rate and copy_per_pixel (capped by the room's rate); no
    rows at all move nothing."""
    bufs = ccdgpu.RowsBuffers(pinned=False, rows_per_pixel=0.5)
    assert bufs.learn(0, 400, 264) is False
    assert (bufs.max_rate, bufs.copy_per_pixel, bufs.rows_per_pixel) == (0.0, None, 0.5)
    assert bufs.learn(200, 400, 264) is False
    assert bufs.max_rate == 200 / 400 and bufs.rows_per_pixel == 0.5
    assert bufs.copy_per_pixel == min(0.5, 1.25 * 200 / 400)
    assert bufs.learn(100, 400, 264) is False  # (a lower rate later: the highest one holds)
    assert bufs.max_rate == 200 / 400 and bufs.copy_per_pixel == 0.5 and bufs.rows_per_pixel == 0.5


def test_rows_buffers_reserve_sizes_the_copy_by_the_learned_rate():
    """RowsBuffers.reserve: room for rows_per_pixel x pixels + 64 rows (grown with headroom), the copy
    that many until a rate is learned, then copy_per_pixel x pixels + 64, never past the room."""
    bufs = ccdgpu.RowsBuffers(pinned=False, rows_per_pixel=2.0)
    room, cap = bufs.reserve(400, 13)
    assert room == bufs.rows.size >= 864 and cap == 864
    assert bufs.offsets.size >= 401 and bufs.mask.size >= 400 * 13
    bufs.learn(400, 400, cap)
    assert bufs.reserve(400, 13) == (room, int(1.25 * 400) + 64)
