"""ctypes binding of libccdgpu.so (include/ccdgpu.h) -- the MI355X change-detection backend.

This is the only way the Python host side reaches the GPU: plain pointers and sizes through the
C-ABI, no torch types.  The library must be built (``__graft_entry__.build()`` / ``make -C
lcmap-firebird_amd``); if it is missing or no gfx950 device is visible, every call raises
``CcdGpuError`` -- there is no CPU fallback on the product path.
"""
import ctypes
import os
import threading

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
UPLOAD_SLOTS = 4  # CCDGPU_UPLOAD_SLOTS (include/ccdgpu.h): input slots per context
LIB_PATH = os.environ.get('CCDGPU_LIBRARY') or os.path.join(os.path.dirname(_HERE), 'lib', 'libccdgpu.so')

_lib = None
_lib_lock = threading.Lock()


class CcdGpuError(RuntimeError):
    def __init__(self, code, message):
        super().__init__('ccdgpu error %d: %s' % (code, message))
        self.code = code
        self.message = message


class QAValueError(ValueError):
    """Unsupported bit-packed QA value: the analogue of pyccd qa.qabitval's ValueError."""


EXPORTS = tuple(abi.SIGNATURES)


def _declare(L):
    """The signatures of abi.SIGNATURES on library ``L``; a symbol it lacks is left for ctypes to name."""
    return abi.declare(L, abi.SIGNATURES)


def lib():
    """Load libccdgpu.so (raises CcdGpuError if it has not been built)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise CcdGpuError(abi.E_HIP, 'libccdgpu.so not built at %s (run __graft_entry__.build())' % LIB_PATH)
            _lib = _declare(ctypes.CDLL(LIB_PATH))
    return _lib


def last_error():
    return lib().ccdgpu_last_error().decode()


def _check(rc):
    if rc == abi.E_QA:
        raise QAValueError(last_error())
    if rc != 0:
        raise CcdGpuError(rc, last_error())


def _params(params):
    """abi.Params: ``params`` itself, or made from a pyccd-style dict (None: the defaults)."""
    return params if isinstance(params, abi.Params) else abi.params_from_dict(params)


def _timed(fn, *args, after=()):
    """(return code, kernel seconds) of a library call whose ``double *kernel_seconds`` follows ``args``."""
    secs = ctypes.c_double(0.0)
    return fn(*(args + (ctypes.byref(secs),) + tuple(after))), secs.value


def _take(rc, out, ok=(0,)):
    """The numpy copy of a library-owned abi.Result / abi.Rows the call that returned ``rc`` filled
    (raising unless rc is in ``ok``); the library's memory is freed either way."""
    L = lib()
    unpack, free = (abi.unpack, L.ccdgpu_result_free) if isinstance(out, abi.Result) else (abi.unpack_rows, L.ccdgpu_rows_free)
    try:
        if rc not in ok:
            _check(rc)
        return unpack(out)
    finally:
        free(ctypes.byref(out))


def _allocator(pinned):
    """``alloc(shape, dtype)``: page-locked arrays (pinned_empty) or numpy's own."""
    return pinned_empty if pinned else np.empty


def _chip_coords(cx, cy, n_chips):
    """cx / cy as int32 arrays of one entry per chip."""
    cx = np.ascontiguousarray(cx, dtype=np.int32)
    cy = np.ascontiguousarray(cy, dtype=np.int32)
    if cx.shape != (n_chips,) or cy.shape != (n_chips,):
        raise ValueError('cx / cy need one entry per chip (%d)' % n_chips)
    return cx, cy


def version():
    return lib().ccdgpu_version().decode()


def device_count():
    n = ctypes.c_int(0)
    rc = lib().ccdgpu_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def device_numa_node(device=0):
    """NUMA node the GPU ``device`` is attached to (-1: not exposed by the platform)."""
    n = ctypes.c_int(-1)
    _check(lib().ccdgpu_device_numa_node(int(device), ctypes.byref(n)))
    return n.value


def default_params():
    p = abi.Params()
    lib().ccdgpu_params_default(ctypes.byref(p))
    return p


class ChipBatch(object):
    """Host buffers of one staged batch in the ccdgpu_stage_chips layout (include/ccdgpu.h):
    chips of their own pixel / observation counts packed back to back.  ``pinned=True``
    allocates them in page-locked memory (ccdgpu_host_alloc) so uploads overlap detection.

        b = ChipBatch([10000, 10000], [1421, 2121], pinned=True)
        d, s, q = b.chip(1)      # views: dates [n], spectra [7][n_pix][n], qa [n_pix][n]
    """

    def __init__(self, n_pix, n_obs, pinned=False, storage=None):
        """``storage``: (dates int64, spectra int16, qa uint16) 1-D arrays of at least the batch's
        sizes (e.g. ``batch_storage``, reused across batches): the batch's arrays are their
        prefixes instead of new allocations."""
        self._init_shape(n_pix, n_obs)
        nd, ns = int(self.obs_off[-1]), int(self.data_off[-1])
        self.storage = storage
        if storage is not None:
            sd, ss, sq = storage
            if sd.dtype != np.int64 or ss.dtype != np.int16 or sq.dtype != np.uint16 or \
                    sd.size < nd or ss.size < 7 * ns or sq.size < ns:
                raise ValueError('storage too small or of the wrong types for this batch')
            self.dates, self.spectra, self.qa = sd[:nd], ss[:7 * ns], sq[:ns]
            return
        alloc = _allocator(pinned)
        self.dates = alloc((nd,), np.int64)
        self.spectra = alloc((7 * ns,), np.int16)
        self.qa = alloc((ns,), np.uint16)

    def _init_shape(self, n_pix, n_obs):
        """The chips' pixel / observation counts and the offsets of their dates, pixels and data."""
        self.n_pix = np.ascontiguousarray(n_pix, dtype=np.int32).reshape(-1)
        self.n_obs = np.ascontiguousarray(n_obs, dtype=np.int32).reshape(-1)
        if self.n_pix.shape != self.n_obs.shape or self.n_pix.size == 0:
            raise ValueError('n_pix and n_obs must be equal-length, non-empty')
        self.obs_off = np.concatenate([[0], np.cumsum(self.n_obs, dtype=np.int64)])
        self.pix_off = np.concatenate([[0], np.cumsum(self.n_pix, dtype=np.int64)])
        self.data_off = np.concatenate([[0], np.cumsum(self.n_pix.astype(np.int64) * self.n_obs)])

    @property
    def n_chips(self):
        return int(self.n_pix.size)

    @property
    def total_pixels(self):
        return int(self.pix_off[-1])

    @property
    def nbytes(self):
        return self.dates.nbytes + self.spectra.nbytes + self.qa.nbytes

    def chip(self, c):
        """Views of chip c: (dates [n], spectra [7][n_pix][n], qa [n_pix][n])."""
        npx, n = int(self.n_pix[c]), int(self.n_obs[c])
        o, d = int(self.obs_off[c]), int(self.data_off[c])
        return (self.dates[o:o + n], self.spectra[7 * d:7 * (d + npx * n)].reshape(7, npx, n),
                self.qa[d:d + npx * n].reshape(npx, n))

    def set_chip(self, c, dates, spectra, qa):
        d, s, q = self.chip(c)
        d[...], s[...], q[...] = dates, spectra, qa

    @classmethod
    def from_chips(cls, chips, pinned=False):
        """[(dates [n], spectra [7][n_pix][n], qa [n_pix][n]), ...] -> ChipBatch."""
        chips = list(chips)
        b = cls([c[2].shape[0] for c in chips], [c[0].shape[0] for c in chips], pinned=pinned)
        for i, (d, s, q) in enumerate(chips):
            b.set_chip(i, d, s, q)
        return b

    def mask_of(self, bits, c):
        """Chip c's int8 [n_pix][n_obs] processing mask from a batch row fetch's bit words."""
        p0, p1 = int(self.pix_off[c]), int(self.pix_off[c + 1])
        return abi.unpack_mask_bits(bits[p0:p1], int(self.n_obs[c]))

    def mask_bits_of(self, bits, c):
        """Chip c's bit words of a batch row fetch, [n_pix][ceil(n_obs / 32)] (no unpacking;
        the batch's own word count, set by its largest chip, is trimmed to the chip's)."""
        return bits[int(self.pix_off[c]):int(self.pix_off[c + 1]), :(int(self.n_obs[c]) + 31) // 32]


class EncodedBatch(ChipBatch):
    """A batch in the transport encoding of ccdgpu_encode_chips (include/ccdgpu.h): the chips'
    dates plus one byte buffer, uploaded with Context.stage_slot_encoded and decoded on the device
    into the ChipBatch layout.  Shape, dates and mask helpers as ChipBatch; chip(c) gives
    (dates, None, None) -- the pixel data exist only in encoded form.

        e = EncodedBatch.encode([(d0, s0, q0), (d1, s1, q1)], storage=encode_storage(...))

    ``pack=True`` (here, in ``fill`` / ``encode`` and in ``encode_storage``): the encodable chips'
    band runs travel bit-packed (mode 2 sections: per (pixel, band) a base, a bit width and an
    exception list) instead of as int16 columns -- fewer bytes, the same device inputs; the batch
    and its storage are then sized by the packed bound.
    """

    def __init__(self, n_pix, n_obs, storage=None, pinned=True, pack=False):
        self._init_shape(n_pix, n_obs)
        self.pack = bool(pack)
        bound = _encoded_bound(self.n_chips, self.n_pix, self.n_obs, self.pack)
        nd = int(self.obs_off[-1])
        self.storage = storage
        if storage is not None:
            sd, sb = storage
            if sd.dtype != np.int64 or sb.dtype != np.uint8 or sd.size < nd or sb.size < bound:
                raise ValueError('storage too small or of the wrong types for this batch')
            self.dates, self.buf = sd[:nd], sb
        else:
            alloc = _allocator(pinned)
            self.dates, self.buf = alloc((nd,), np.int64), alloc((bound,), np.uint8)
        self.spectra = self.qa = None
        self.bound = bound
        self.nbytes_encoded = 0

    @property
    def nbytes(self):
        return self.dates.nbytes + self.nbytes_encoded

    def chip(self, c):
        n, o = int(self.n_obs[c]), int(self.obs_off[c])
        return self.dates[o:o + n], None, None

    def set_chip(self, c, dates, spectra, qa):
        raise TypeError('EncodedBatch holds encoded chips: build it with EncodedBatch.encode')

    def fill(self, chips, threads=4, drop_bits=1, strict_bits=1, pack=None):
        """Encode chips [(dates [n], spectra [7][n_pix][n] int16, qa [n_pix][n] uint16), ...]
        (any C-contiguous arrays: pinned batch views, or a source's own arrays -- nothing else is
        copied) into this batch; returns the encoded bytes.  ``drop_bits`` / ``strict_bits``:
        QA bits whose observations send no band values / must hold -9999 (include/ccdgpu.h; the
        default, the fill bit for both, is lossless; ``unread_drop_bits(params)`` gives the bits of
        observations the detection never reads).  ``pack`` (default: the batch's own setting)
        selects the bit-packed mode 2; a batch built without it may be too small for it."""
        pack = self.pack if pack is None else bool(pack)
        chips = list(chips)
        if len(chips) != self.n_chips:
            raise ValueError('%d chips for a batch of %d' % (len(chips), self.n_chips))
        sp = (ctypes.c_void_p * len(chips))()
        qp = (ctypes.c_void_p * len(chips))()
        keep = []
        for i, (d, s, q) in enumerate(chips):
            d = np.asarray(d)
            s = np.ascontiguousarray(s, dtype=np.int16)
            q = np.ascontiguousarray(q, dtype=np.uint16)
            if d.shape != (int(self.n_obs[i]),) or s.shape != (7, int(self.n_pix[i]), int(self.n_obs[i])) or \
                    q.shape != (int(self.n_pix[i]), int(self.n_obs[i])):
                raise ValueError('chip %d does not have this batch\'s shape' % i)
            o = int(self.obs_off[i])
            self.dates[o:o + d.shape[0]] = d
            sp[i], qp[i] = s.ctypes.data, q.ctypes.data
            keep.append((s, q))
        args = (self.n_chips, self.n_pix.ctypes.data, self.n_obs.ctypes.data, ctypes.cast(sp, ctypes.c_void_p),
                ctypes.cast(qp, ctypes.c_void_p), self.buf.ctypes.data, self.buf.size, int(threads), int(drop_bits),
                int(strict_bits))
        if pack:
            n = int(lib().ccdgpu_encode_chips_flags(*(args + (abi.ENC_PACK,))))
        else:
            n = int(lib().ccdgpu_encode_chips(*args))
        if n < 0:
            raise ValueError('ccdgpu_encode_chips failed (%d)' % n)
        self.nbytes_encoded = n
        return n

    @classmethod
    def encode(cls, chips, threads=4, storage=None, pinned=True, drop_bits=1, strict_bits=1, pack=False):
        chips = list(chips)
        b = cls([c[2].shape[0] for c in chips], [c[0].shape[0] for c in chips], storage=storage, pinned=pinned,
                pack=pack)
        b.fill(chips, threads, drop_bits, strict_bits)
        return b

    def check(self):
        """The header / layout checks of the upload (ccdgpu_encoded_check; no device needed):
        raises CcdGpuError naming the first problem."""
        _check(lib().ccdgpu_encoded_check(self.n_chips, self.n_pix.ctypes.data, self.n_obs.ctypes.data,
                                          self.buf.ctypes.data, int(self.nbytes_encoded)))

    def chip_modes(self):
        """Per chip: 1 if encoded, 2 if encoded with bit-packed band runs, 0 if sent raw (from
        the section headers)."""
        off = self.buf[8:8 * (self.n_chips + 2)].view(np.int64)
        return [int(self.buf[int(o):int(o) + 4].view(np.int32)[0]) for o in off[:self.n_chips]]


def _encoded_bound(n_chips, n_pix, n_obs, pack):
    if pack:
        return int(lib().ccdgpu_encoded_bound_flags(n_chips, n_pix.ctypes.data, n_obs.ctypes.data, abi.ENC_PACK))
    return int(lib().ccdgpu_encoded_bound(n_chips, n_pix.ctypes.data, n_obs.ctypes.data))


def encode_storage(max_chips, max_pix, max_obs, pinned=True, pack=False):
    """Reusable buffers for EncodedBatch(..., storage=...): room for ``max_chips`` chips of up to
    ``max_pix`` pixels x ``max_obs`` observations (``pack``: of the bit-packed mode 2)."""
    n = int(max_chips)
    np_ = np.full(n, int(max_pix), dtype=np.int32)
    no = np.full(n, int(max_obs), dtype=np.int32)
    bound = _encoded_bound(n, np_, no, pack)
    alloc = _allocator(pinned)
    return alloc((n * int(max_obs),), np.int64), alloc((bound,), np.uint8)


def unread_drop_bits(params=None):
    """(drop_bits, strict_bits) for the transport encoding that drops every band value the
    detection never reads: observations whose QA word has the fill, cloud or shadow bit (qabitval
    classes them as fill / cloud / shadow whatever else is set, and no procedure keeps those
    classes); fill observations stay strict (their bands must be -9999).  For non-bit-packed QA
    (class values, not bits) only the lossless (fill bit 0) setting applies."""
    p = _params(params)
    if not p.qa_bitpacked:
        return 0, 0
    bits = [int(p.qa_fill), int(p.qa_cloud), int(p.qa_shadow)]
    if any(b < 0 or b > 15 for b in bits):
        return 0, 0  # (bits outside a 16-bit word: nothing dropped)
    drop = 0
    for b in bits:
        drop |= 1 << b
    return drop, 1 << int(p.qa_fill)


def encode_vector_path():
    """True if the encoder uses AVX-512 VBMI2 compress-stores on this CPU."""
    return bool(lib().ccdgpu_encode_vector_path())


def _as_inputs(dates, spectra, qa):
    dates = np.ascontiguousarray(dates, dtype=np.int64)
    spectra = np.ascontiguousarray(spectra, dtype=np.int16)
    qa = np.ascontiguousarray(qa, dtype=np.uint16)
    return dates, spectra, qa


def _predict_dates(dates):
    return np.ascontiguousarray(dates, dtype=np.int64).reshape(-1)


def _predict_modes(cover, dtype):
    """cover 'span' / 'extend' and dtype 'float32' / 'int16' (or numpy's) -> the library's codes;
    integers pass through for the library to check."""
    if not isinstance(cover, (int, np.integer)):
        if cover not in abi.COVERS:
            raise ValueError("cover must be 'span' or 'extend', not %r" % (cover,))
        cover = abi.COVERS[cover]
    if not isinstance(dtype, (int, np.integer)):
        name = dtype if isinstance(dtype, str) else np.dtype(dtype).name
        if name not in abi.PREDICT_DTYPES:
            raise ValueError("dtype must be 'float32' or 'int16', not %r" % (dtype,))
        dtype = abi.PREDICT_DTYPES[name]
    return int(cover), int(dtype)


def _predict_buffers(out, seg_index, n_pix, n_dates, dtype):
    """(values, seg_index or None) to fill: the caller's arrays, checked, or new ones."""
    want = np.dtype(np.int16 if dtype == abi.PREDICT_I16 else np.float32)
    for a, shape, typ, name in ((out, (abi.NBANDS, n_pix, n_dates), want, 'out'),
                                (seg_index, (n_pix, n_dates), np.dtype(np.int32), 'seg_index')):
        if isinstance(a, np.ndarray) and (a.shape != shape or a.dtype != typ or not a.flags.c_contiguous or not a.flags.writeable):
            raise ValueError('%s must be a writeable C-contiguous %s array of shape %r, got %s %r'
                             % (name, typ.name, shape, a.dtype.name, a.shape))
    if out is None:
        out = np.empty((abi.NBANDS, n_pix, n_dates), dtype=want)
    elif not isinstance(out, np.ndarray):
        raise ValueError('out must be a numpy array or None')
    if isinstance(seg_index, np.ndarray):
        return out, seg_index
    return out, (np.empty((n_pix, n_dates), dtype=np.int32) if seg_index else None)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _row_table(row_offsets, rows):
    """(row_offsets int64 [n_pix + 1], rows abi.ROW_DTYPE) of a host table of segment rows, checked
    against each other."""
    off = np.ascontiguousarray(row_offsets, dtype=np.int64).reshape(-1)
    r = np.ascontiguousarray(rows, dtype=abi.ROW_DTYPE).reshape(-1)
    if off.shape[0] < 1:
        raise ValueError('row_offsets must have n_pix + 1 entries')
    if int(off[-1]) != r.shape[0]:
        raise ValueError('row_offsets end at %d, the table has %d rows' % (int(off[-1]), r.shape[0]))
    return off, r


def _check_args(row_offsets, rows, dates, n_pix, n_rows):
    """The table and date arguments of ccdgpu_predict_check / ccdgpu_products_check from array-likes
    that may be None (a NULL pointer): ((n_pix, row_offsets, n_rows, rows), (n_dates, dates), the
    arrays the pointers point into).  n_pix / n_rows default to the arrays' sizes."""
    off = None if row_offsets is None else np.ascontiguousarray(row_offsets, dtype=np.int64).reshape(-1)
    r = None if rows is None else np.ascontiguousarray(rows, dtype=abi.ROW_DTYPE).reshape(-1)
    d = None if dates is None else _predict_dates(dates)
    if n_pix is None:
        n_pix = 0 if off is None else off.shape[0] - 1
    if n_rows is None:
        n_rows = 0 if r is None else r.shape[0]
    n_dates = 1 if d is None else d.shape[0]  # (a NULL date vector of no dates is fine: ask for one)
    if off is not None and off.shape[0] < n_pix + 1:
        raise ValueError('row_offsets has %d entries, n_pix + 1 is %d' % (off.shape[0], n_pix + 1))
    return (int(n_pix), _ptr(off), int(n_rows), _ptr(r)), (int(n_dates), _ptr(d)), (off, r, d)


def predict_check(row_offsets, rows, dates, avg_days_yr=365.2425, cover=0, dtype=0, n_pix=None, n_rows=None):
    """ccdgpu_predict_check (no device needed) over array-likes; None passes a NULL pointer, n_pix
    / n_rows default to the arrays' sizes.  Raises ValueError with the library's message."""
    table, when, keep = _check_args(row_offsets, rows, dates, n_pix, n_rows)  # (keep: alive over the call)
    if lib().ccdgpu_predict_check(*(table + when + (float(avg_days_yr), int(cover), int(dtype)))) != 0:
        raise ValueError(last_error())


def year_window(dates):
    """(a, b) int64 arrays: the ordinals of 1 January of each date's calendar year and of the next
    1 January (ccdgpu_year_window; no device needed).  Raises ValueError for a date outside
    1 .. abi.PREDICT_MAX_DATE."""
    d = _predict_dates(dates)
    a, b = np.empty_like(d), np.empty_like(d)
    L = lib()
    x, y = ctypes.c_int64(0), ctypes.c_int64(0)
    for i, t in enumerate(d.tolist()):
        if L.ccdgpu_year_window(t, ctypes.byref(x), ctypes.byref(y)) != 0:
            raise ValueError(last_error())
        a[i], b[i] = x.value, y.value
    return a, b


def product_params(bot=None, mag_bands=None, cover='extend', n_classes=0, labels=None):
    """abi.ProductParams from the library's defaults (ccdgpu_product_params_default) and what is given:
    cover 'span' / 'extend' (or the code), labels the product values of the classes (default k + 1;
    n_classes then defaults to their number)."""
    p = abi.ProductParams()
    lib().ccdgpu_product_params_default(ctypes.byref(p))
    if bot is not None:
        p.bot = int(bot)
    if mag_bands is not None:
        p.mag_bands = int(mag_bands)
    p.cover = _predict_modes(cover, abi.PREDICT_F32)[0]
    if labels is not None:
        labels = [int(v) for v in labels]
        if len(labels) > abi.PRODUCT_MAX_CLASSES or any(not 0 <= v <= 255 for v in labels):
            raise ValueError('labels must be at most %d values in 0 .. 255' % abi.PRODUCT_MAX_CLASSES)
        for k, v in enumerate(labels):
            p.labels[k] = v
        if not n_classes:
            n_classes = len(labels)
    p.n_classes = int(n_classes)
    return p


def _product_request(want, out, n_pix, n_dates, cover_ok):
    """(names, arrays dict, abi.Products) of a product request: ``want`` names (None: the change
    products, and the cover products when there is an rfrawp), ``out`` an optional dict of arrays
    [n_dates][n_pix] to fill instead of new ones."""
    if want is None:
        want = abi.CHANGE_PRODUCTS + (abi.COVER_PRODUCTS if cover_ok else ())
    want = (want,) if isinstance(want, str) else tuple(want)
    for name in want:
        if name not in abi.PRODUCT_DTYPES:
            raise ValueError('unknown product %r (one of %s)' % (name, ', '.join(n for n, _ in abi.PRODUCTS)))
    arrays, ptrs = {}, abi.Products()
    for name, typ in abi.PRODUCTS:
        if name not in want:
            continue
        a = None if out is None else out.get(name)
        if a is None:
            a = np.empty((n_dates, n_pix), dtype=typ)
        elif (not isinstance(a, np.ndarray) or a.shape != (n_dates, n_pix) or a.dtype != np.dtype(typ) or
              not a.flags.c_contiguous or not a.flags.writeable):
            raise ValueError('out[%r] must be a writeable C-contiguous %s array of shape %r'
                             % (name, np.dtype(typ).name, (n_dates, n_pix)))
        arrays[name] = a
        setattr(ptrs, name, a.ctypes.data)
    return want, arrays, ptrs


def _rfrawp(rfrawp, n_rows, params):
    """rfrawp as float32 [n_rows][n_classes] (n_classes of the params set from it when 0), or None."""
    if rfrawp is None:
        return None
    r = np.ascontiguousarray(rfrawp, dtype=np.float32)
    if r.ndim != 2 or r.shape[0] != n_rows:
        raise ValueError('rfrawp must be [%d][n_classes], got %r' % (n_rows, r.shape))
    if params.n_classes == 0:
        params.n_classes = r.shape[1]
    if r.shape[1] != params.n_classes:
        raise ValueError('rfrawp has %d classes, the parameters %d' % (r.shape[1], params.n_classes))
    return r


def products_check(row_offsets, rows, dates, rfrawp=None, params=None, want=abi.CHANGE_PRODUCTS, n_pix=None, n_rows=None):
    """ccdgpu_products_check (no device needed) over array-likes; None passes a NULL pointer (for
    ``params`` the defaults), n_pix / n_rows default to the arrays' sizes; ``want`` names the outputs
    that are requested (as non-NULL pointers that are not written).  Raises ValueError with the
    library's message."""
    table, when, keep = _check_args(row_offsets, rows, dates, n_pix, n_rows)  # (keep: alive over the call)
    rf = None if rfrawp is None else np.ascontiguousarray(rfrawp, dtype=np.float32)
    p = product_params() if params is None else params
    ptrs = abi.Products()
    for name in want:
        setattr(ptrs, name, 1)
    if lib().ccdgpu_products_check(*(table + (_ptr(rf),) + when + (None if params is False else ctypes.byref(p),
                                                                     ctypes.byref(ptrs)))) != 0:
        raise ValueError(last_error())


def train_params(n_trees=None, max_depth=None, features_per_node=None, min_instances_per_node=None, min_info_gain=None,
                 bootstrap=None, seed=None):
    """abi.TrainParams from the library's defaults (ccdgpu_train_params_default: 500 trees, depth 5, the
    sqrt subset, bootstrap, seed 0) and what is given; features_per_node 0 or 'sqrt' is Spark's sqrt,
    'all' every feature."""
    p = abi.TrainParams()
    lib().ccdgpu_train_params_default(ctypes.byref(p))
    if features_per_node in ('sqrt', 'all'):
        features_per_node = 0 if features_per_node == 'sqrt' else abi.FOREST_MAX_FEATURES
    for name, v in (('n_trees', n_trees), ('max_depth', max_depth), ('features_per_node', features_per_node),
                    ('min_instances_per_node', min_instances_per_node), ('bootstrap', bootstrap), ('seed', seed)):
        if v is not None:
            setattr(p, name, int(v))
    if min_info_gain is not None:
        p.min_info_gain = float(min_info_gain)
    return p


def _train_args(x, labels, edges, n_classes, params):
    """The arguments of ccdgpu_train_check / ccdgpu_forest_train after the context, from array-likes:
    x [n_rows][n_features], labels [n_rows], edges one sequence per feature (packed back to back for the
    library), n_classes (None: max(label) + 1), params an abi.TrainParams or a dict for ``train_params``.
    Returns (arguments, the arrays they point into)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    if x.ndim != 2 or x.shape[0] != y.shape[0]:
        raise ValueError('x must be [n_rows][n_features] and labels [n_rows], got %r and %r' % (x.shape, y.shape))
    if len(edges) != x.shape[1]:
        raise ValueError('edges must hold one sequence per feature: %d, not %d' % (x.shape[1], len(edges)))
    per = [np.asarray(e, dtype=np.float64).reshape(-1) for e in edges]
    n_edges = np.array([e.shape[0] for e in per], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate(per) if per else np.zeros(0), dtype=np.float64)
    if n_classes is None:
        n_classes = int(y.max()) + 1 if y.size else 0
    p = params if isinstance(params, abi.TrainParams) else train_params(**(params or {}))
    return ((x.ctypes.data, y.ctypes.data, x.shape[0], x.shape[1], int(n_classes), flat.ctypes.data, n_edges.ctypes.data,
             ctypes.byref(p)), (x, y, flat, n_edges, p))


def train_check(x, labels, edges, n_classes=None, **params):
    """ccdgpu_train_check (no device needed) over array-likes, as ``Context.train_forest`` takes them.
    Raises ValueError with the library's message."""
    args, keep = _train_args(x, labels, edges, n_classes, params)  # (keep: alive over the call)
    if lib().ccdgpu_train_check(*args) != 0:
        raise ValueError(last_error())


def _splits_args(x, max_bins):
    """The arguments of ccdgpu_splits_check / ccdgpu_forest_find_splits between the context and the
    outputs, from x [n_rows][n_features]; returns (arguments, the array they point into)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError('x must be [n_rows][n_features], got %r' % (x.shape,))
    return (x.ctypes.data, x.shape[0], x.shape[1], int(max_bins)), x


def splits_check(x, max_bins=32):
    """ccdgpu_splits_check (no device needed) over an array-like, as ``Context.find_splits`` takes it.
    Raises ValueError with the library's message."""
    args, keep = _splits_args(x, max_bins)  # (keep: alive over the call)
    if lib().ccdgpu_splits_check(*args) != 0:
        raise ValueError(last_error())


class _Staged(object):
    """The shape of a staged batch, one record for every staging form: the host arrays to keep
    alive, the chips' pixel and observation counts, and whether the batch is a ChipBatch (an
    EncodedBatch too) rather than uniform arrays.  ``_Staged()`` is "nothing staged"."""

    def __init__(self, keep=None, n_pix=(), n_obs=(), is_batch=False):
        self.keep = keep
        self.n_pix = np.asarray(n_pix, dtype=np.int32).reshape(-1)
        self.n_obs = np.asarray(n_obs, dtype=np.int32).reshape(-1)
        self.is_batch = is_batch

    @classmethod
    def uniform(cls, keep, n_chips, n_pix, n_obs):
        """``n_chips`` chips of (n_pix, n_obs) each: stage / stage_slot / stage_chipmunk / detect_batch."""
        return cls(keep, [n_pix] * n_chips, [n_obs] * n_chips)

    @classmethod
    def of_batch(cls, batch):
        return cls(batch, batch.n_pix, batch.n_obs, True)

    @property
    def n_chips(self):
        return int(self.n_pix.size)

    @property
    def total_pixels(self):
        """Pixels of the whole batch; None with nothing staged."""
        return None if self.keep is None else int(self.n_pix.sum(dtype=np.int64))

    @property
    def mask_words(self):
        """uint32 words per pixel of a batch row fetch's mask: set by the chip with most observations."""
        return (int(self.n_obs.max()) + 31) // 32

    def chip_pixels(self, chip):
        """Pixels of chip ``chip``; None for no such chip, or with nothing staged."""
        return int(self.n_pix[chip]) if 0 <= chip < self.n_chips else None


class Context(object):
    """One HIP device + stream (ccdgpu_ctx).  Not shared across threads."""

    def __init__(self, device=0, copy_cus=0):
        """copy_cus > 0 reserves that many CUs for the context's copy stream (upload decode,
        blits), the rest for detection (ccdgpu_init_copy_cus, include/ccdgpu.h)."""
        self.qa_error = False
        self._ctx = ctypes.c_void_p()
        self._last = _Staged()     # the batch of the last run (of stage / stage_chips: as soon as staged)
        self._slots = {}           # input slot -> _Staged of the batch uploaded into it
        self._pending_slot = None  # slot of a run_slot_begin* without its run_slot_end* yet
        self._rows_req = None      # (cx, cy, bufs, width, n_pix, words, cap) of a run_slot_begin_rows
        self._forest_shape = None  # (n_features, n_classes) of the forest set
        self._forest_trees = 0     # and its tree count
        self.forest_seconds = self.train_seconds = self.predict_seconds = self.products_seconds = self.oob_seconds = 0.0
        self.permutation_seconds = self.splits_seconds = 0.0
        self.forest_rows = 0
        if copy_cus:
            _check(lib().ccdgpu_init_copy_cus(int(device), int(copy_cus), ctypes.byref(self._ctx)))
        else:
            _check(lib().ccdgpu_init(int(device), ctypes.byref(self._ctx)))
        self.device = device

    def _finish(self, rc):
        """End of a run: raise on failure; an unsupported QA value leaves results (the pixel's
        procedure is -1 in fetch) and sets ``qa_error``."""
        if rc not in (0, abi.E_QA):
            _check(rc)
        self.qa_error = rc == abi.E_QA

    def _chip_pixels(self, chip, probe, message):
        """Pixels of chip ``chip`` of the last run.  Nothing staged here, or no such chip: ``probe()`` -- the
        library call without buffers -- raises with the library's reason, or else ``message`` is raised."""
        n_pix = self._last.chip_pixels(chip)
        if n_pix is None:
            probe()
            raise CcdGpuError(abi.E_INVAL, message)
        return n_pix

    def close(self):
        if self._ctx:
            lib().ccdgpu_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().ccdgpu_synchronize(self._ctx))

    def detect_batch(self, dates, spectra, qa, params=None):
        """Pixels sharing one date vector: dates [n], spectra [7][n_pix][n], qa [n_pix][n].
        Returns abi.Unpacked.  Raises QAValueError on unsupported QA values."""
        dates, spectra, qa = _as_inputs(dates, spectra, qa)
        n_pix, n_obs = qa.shape
        if spectra.shape != (7, n_pix, n_obs) or dates.shape != (n_obs,):
            raise ValueError('shape mismatch: dates %s spectra %s qa %s' % (dates.shape, spectra.shape, qa.shape))
        p = _params(params)
        res = abi.Result()
        rc = lib().ccdgpu_detect_batch(self._ctx, ctypes.byref(p), n_pix, n_obs, dates.ctypes.data,
                                       spectra.ctypes.data, qa.ctypes.data, ctypes.byref(res))
        if rc in (0, abi.E_QA):  # the context's last run is now this one-chip batch (predict_rows sizes its output by it)
            self._last = _Staged.uniform((dates, spectra, qa), 1, n_pix, n_obs)
        u = _take(rc, res, ok=(0, abi.E_QA))
        if rc == abi.E_QA:
            err = QAValueError(last_error())
            err.result = u
            raise err
        return u

    # device-resident path ------------------------------------------------------------------
    def stage(self, dates, spectra, qa, params=None):
        """dates [C][n], spectra [C][7][n_pix][n], qa [C][n_pix][n] -> staged on the device."""
        dates, spectra, qa = _as_inputs(dates, spectra, qa)
        n_chips, n_pix, n_obs = qa.shape
        p = _params(params)
        _check(lib().ccdgpu_stage(self._ctx, ctypes.byref(p), n_chips, n_pix, n_obs,
                                  dates.ctypes.data, spectra.ctypes.data, qa.ctypes.data))
        self._last = _Staged.uniform((dates, spectra, qa), n_chips, n_pix, n_obs)

    def stage_chips(self, batch, params=None):
        """Stage a ChipBatch (or a list of (dates, spectra, qa) chips of any sizes) in one
        batch: ccdgpu_stage_chips."""
        if not isinstance(batch, ChipBatch):
            batch = ChipBatch.from_chips(batch)
        p = _params(params)
        _check(lib().ccdgpu_stage_chips(self._ctx, ctypes.byref(p), batch.n_chips, batch.n_pix.ctypes.data,
                                        batch.n_obs.ctypes.data, batch.dates.ctypes.data,
                                        batch.spectra.ctypes.data, batch.qa.ctypes.data))
        self._last = _Staged.of_batch(batch)
        return batch

    def stage_slot_chips(self, slot, batch, params=None):
        """Upload a ChipBatch into input slot 0 .. UPLOAD_SLOTS-1 on the copy stream and return at once (the
        batch must stay alive and unchanged until run_slot(slot) returns; pinned=True batches
        upload asynchronously).  An EncodedBatch goes through stage_slot_encoded."""
        if isinstance(batch, EncodedBatch):
            return self.stage_slot_encoded(slot, batch, params)
        p = _params(params)
        _check(lib().ccdgpu_stage_slot_chips(self._ctx, int(slot), ctypes.byref(p), batch.n_chips,
                                             batch.n_pix.ctypes.data, batch.n_obs.ctypes.data,
                                             batch.dates.ctypes.data, batch.spectra.ctypes.data,
                                             batch.qa.ctypes.data))
        self._slots[int(slot)] = _Staged.of_batch(batch)

    def stage_slot_encoded(self, slot, batch, params=None):
        """Upload an EncodedBatch into input slot ``slot`` and decode it there on the device (copy
        stream; same life-time rules as stage_slot_chips)."""
        p = _params(params)
        _check(lib().ccdgpu_stage_slot_encoded(self._ctx, int(slot), ctypes.byref(p), batch.n_chips,
                                               batch.n_pix.ctypes.data, batch.n_obs.ctypes.data,
                                               batch.dates.ctypes.data, batch.buf.ctypes.data,
                                               int(batch.nbytes_encoded)))
        self._slots[int(slot)] = _Staged.of_batch(batch)

    def _last_batch_coords(self, cx, cy):
        """(cx, cy) int32 per chip of the last run, which must be of a ChipBatch."""
        if not self._last.is_batch:
            raise ValueError('fetch_batch_rows needs a stage_chips / stage_slot_chips batch')
        return _chip_coords(cx, cy, self._last.n_chips)

    def fetch_batch_rows(self, cx, cy, width=100):
        """Rows of every chip of the last run in one device pass and one copy: (row_offsets
        [total_pixels+1], rows abi.ROW_DTYPE, mask bit words uint32 [total_pixels][words] --
        ChipBatch.mask_of(bits, c) is chip c's int8 [n_pix][n_obs] mask)."""
        cx, cy = self._last_batch_coords(cx, cy)
        r = abi.Rows()
        return _take(lib().ccdgpu_fetch_batch_rows(self._ctx, cx.ctypes.data, cy.ctypes.data, int(width), ctypes.byref(r)),
                     r)

    def fetch_batch_rows_into(self, cx, cy, bufs, width=100):
        """fetch_batch_rows into ``bufs`` (a RowsBuffers, reused across batches: pinned, so the
        rows and mask words arrive by DMA with no host copy; ccdgpu_fetch_batch_rows_into).
        Returns views of its arrays, valid until its next use."""
        cx, cy = self._last_batch_coords(cx, cy)
        L = lib()
        n_pix, words = self._last.total_pixels, self._last.mask_words
        bufs.ensure(n_pix + 1, n_pix * 2, n_pix * words)
        nr = ctypes.c_int64(0)
        for _ in range(2):
            rc = L.ccdgpu_fetch_batch_rows_into(self._ctx, cx.ctypes.data, cy.ctypes.data, int(width),
                                                bufs.offsets.ctypes.data, bufs.offsets.size, bufs.rows.ctypes.data,
                                                bufs.rows.size, bufs.mask.ctypes.data, bufs.mask.size, ctypes.byref(nr))
            if rc == 0:
                break
            if rc != abi.E_INVAL or nr.value <= bufs.rows.size:
                _check(rc)
            bufs.ensure(n_pix + 1, nr.value, n_pix * words)  # more rows than the first guess
        else:
            _check(rc)
        return bufs.offsets[:n_pix + 1], bufs.rows[:nr.value], bufs.mask[:n_pix * words].reshape(n_pix, words)

    def stage_slot(self, slot, dates, spectra, qa, params=None):
        """Upload a batch into input slot 0 .. UPLOAD_SLOTS-1 on the copy stream and return at once (the arrays
        must stay alive and unchanged until run_slot(slot) returns; pinned arrays from
        ``pinned_empty`` make the upload overlap a running detection)."""
        dates, spectra, qa = _as_inputs(dates, spectra, qa)
        n_chips, n_pix, n_obs = qa.shape
        p = _params(params)
        _check(lib().ccdgpu_stage_slot(self._ctx, int(slot), ctypes.byref(p), n_chips, n_pix, n_obs,
                                       dates.ctypes.data, spectra.ctypes.data, qa.ctypes.data))
        self._slots[int(slot)] = _Staged.uniform((dates, spectra, qa), n_chips, n_pix, n_obs)

    def _ran_slot(self, slot):
        """The last run is now the batch of slot ``slot``."""
        self._last = self._slots.get(slot, _Staged())

    def run_slot(self, slot):
        """Detect the batch of input slot ``slot`` (waits for its upload); fetch / fetch_rows as
        after run().  Returns the kernel seconds."""
        rc, secs = _timed(lib().ccdgpu_run_slot, self._ctx, int(slot))
        self._finish(rc)
        self._ran_slot(int(slot))
        return secs

    def run_slot_begin(self, slot):
        """run_slot in halves (ccdgpu_run_slot_begin / _query / _end): launch the detection of
        slot ``slot`` and return at once; run_done() says whether it has completed, and
        run_slot_end() waits for it and finishes as run_slot does.  In between, only stage_slot*
        of other slots may be called."""
        _check(lib().ccdgpu_run_slot_begin(self._ctx, int(slot)))
        self._pending_slot = int(slot)

    def run_done(self):
        rc = lib().ccdgpu_run_query(self._ctx)
        if rc < 0:
            _check(rc)
        return rc == 1

    def run_slot_begin_rows(self, slot, cx, cy, bufs, width=100):
        """run_slot_begin with the batch's rows in the same device chain
        (ccdgpu_run_slot_begin_rows): chip c's rows at (cx[c], cy[c]) land in ``bufs`` (a
        RowsBuffers, grown here to the slot's pixels: offsets, mask words, and rows for
        ``rows_per_pixel`` per pixel); run_slot_end_rows() waits once and returns them."""
        staged = self._slots.get(int(slot), _Staged())
        if not staged.is_batch:
            raise ValueError('run_slot_begin_rows needs a stage_slot_chips / stage_slot_encoded batch')
        cx, cy = _chip_coords(cx, cy, staged.n_chips)
        n_pix, words = staged.total_pixels, staged.mask_words
        _, cap = bufs.reserve(n_pix, words)
        _check(lib().ccdgpu_run_slot_begin_rows(self._ctx, int(slot), cx.ctypes.data, cy.ctypes.data, int(width),
                                                bufs.offsets.ctypes.data, bufs.offsets.size, bufs.rows.ctypes.data,
                                                cap, bufs.mask.ctypes.data, bufs.mask.size))
        self._pending_slot = int(slot)
        self._rows_req = (cx, cy, bufs, int(width), n_pix, words, cap)

    def run_slot_end_rows(self):
        """(row_offsets [n_pix+1], rows, mask words [n_pix][words]) of the batch begun with
        run_slot_begin_rows -- views of its RowsBuffers, valid until their next use.  More rows
        than the buffer held: the buffer grows (and learns the rate) and the rows are fetched."""
        nr = ctypes.c_int64(0)
        rc, _ = _timed(lib().ccdgpu_run_slot_end_rows, self._ctx, after=(ctypes.byref(nr),))
        cx, cy, bufs, width, n_pix, words, cap = self._rows_req
        self._rows_req = None
        self._ran_slot(self._pending_slot)
        # the library sets the count only for a completed run: more rows than the copy held come with
        # E_OVERFLOW, or with E_QA for a batch that also has an unsupported QA value (it still raises)
        if bufs.learn(nr.value, n_pix, cap) and rc in (abi.E_OVERFLOW, abi.E_QA) and self._last.keep is not None:
            self.qa_error = rc == abi.E_QA
            return self.fetch_batch_rows_into(cx, cy, bufs, width)
        self._finish(rc)
        n = nr.value
        return bufs.offsets[:n_pix + 1], bufs.rows[:n], bufs.mask[:n_pix * words].reshape(n_pix, words)

    def run_slot_end(self):
        rc, secs = _timed(lib().ccdgpu_run_slot_end, self._ctx)
        self._finish(rc)
        self._ran_slot(self._pending_slot)
        return secs

    def stage_chipmunk(self, dates, text, offsets, n_pix, params=None):
        """Stage chips from the chipmunk wire format (see ccdc.chipmunk.pack_text):
        dates [C][n] int64, text bytes (concatenated base64 payloads), offsets [C][n][8] int64
        byte offsets of each layer's payload (-1 = missing layer).  Decoding and the pivot to
        the detection layout run on the device; returns the unpack kernel time in seconds."""
        dates = np.ascontiguousarray(dates, dtype=np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if dates.ndim == 1:
            dates = dates[None]
        if offsets.ndim == 2:
            offsets = offsets[None]
        n_chips, n_obs = dates.shape
        if offsets.shape != (n_chips, n_obs, 8):
            raise ValueError('offsets must be [n_chips][n_obs][8], got %r' % (offsets.shape,))
        text = bytes(text)
        p = _params(params)
        rc, secs = _timed(lib().ccdgpu_stage_chipmunk, self._ctx, ctypes.byref(p), n_chips, int(n_pix), n_obs,
                          dates.ctypes.data, text, len(text), offsets.ctypes.data)
        _check(rc)
        self._last = _Staged.uniform((dates, text, offsets), n_chips, int(n_pix), n_obs)
        return secs

    def staged_inputs(self):
        """The staged pixel inputs copied back: (spectra [C][7][n_pix][n], qa [C][n_pix][n]) for
        a uniform batch, flat (spectra, qa) in the ChipBatch layout for a stage_chips batch."""
        s = self._last
        if s.keep is None:
            raise CcdGpuError(abi.E_INVAL, 'nothing staged')
        if s.is_batch:  # (an EncodedBatch too: decoded on the device)
            nd = int((s.n_pix.astype(np.int64) * s.n_obs).sum())
            spectra, qa = np.empty(7 * nd, dtype=np.int16), np.empty(nd, dtype=np.uint16)
        else:
            n_pix, n_obs = int(s.n_pix[0]), int(s.n_obs[0])
            spectra = np.empty((s.n_chips, 7, n_pix, n_obs), dtype=np.int16)
            qa = np.empty((s.n_chips, n_pix, n_obs), dtype=np.uint16)
        _check(lib().ccdgpu_staged_inputs(self._ctx, spectra.ctypes.data, qa.ctypes.data))
        return spectra, qa

    def run(self):
        rc, secs = _timed(lib().ccdgpu_run_staged, self._ctx)
        self._finish(rc)
        return secs

    def fetch(self, chip):
        res = abi.Result()
        return _take(lib().ccdgpu_fetch_staged(self._ctx, int(chip), ctypes.byref(res)), res)

    def fetch_rows(self, chip, cx, cy, width=100):
        """Segment / pixel table rows of staged chip ``chip`` (output writer, packed on the
        device): (row_offsets [n_pix+1], rows abi.ROW_DTYPE [n_rows], mask int8 [n_pix][n_obs])."""
        r = abi.Rows()
        return _take(lib().ccdgpu_fetch_rows(self._ctx, int(chip), int(cx), int(cy), int(width), ctypes.byref(r)), r)

    # random-forest classification of segment rows (rfrawp) --------------------------------------
    def set_forest(self, forest):
        """Make ``forest`` (an abi.Forest, or anything with ``.struct()`` giving one -- a
        ccdc.randomforest.Forest) the context's forest: checked, uploaded, replacing any previous
        one (ccdgpu_forest_set).  Raises ValueError for a forest that fails the check."""
        f = forest if isinstance(forest, abi.Forest) else forest.struct()
        rc = lib().ccdgpu_forest_set(self._ctx, ctypes.byref(f))
        if rc == abi.E_INVAL:
            raise ValueError(last_error())
        _check(rc)
        self._forest_shape = (int(f.n_features), int(f.n_classes))
        self._forest_trees = int(f.n_trees)
        self.forest_seconds = 0.0

    def clear_forest(self):
        _check(lib().ccdgpu_forest_clear(self._ctx))
        self._forest_shape = None
        self._forest_trees = 0

    def _forest_dims(self):
        """(n_features, n_classes) of the forest set."""
        if self._forest_shape is None:
            raise CcdGpuError(abi.E_INVAL, 'no forest set (Context.set_forest)')
        return self._forest_shape

    def classify(self, features):
        """features [n_rows][n_features] float64 (ccdc.features.matrix) -> rfrawp float32
        [n_rows][n_classes] (ccdgpu_classify); the kernel seconds are in ``forest_seconds``."""
        nf, nc = self._forest_dims()
        x = np.ascontiguousarray(features, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != nf:
            raise ValueError('features must be [n_rows][%d], got %r' % (nf, x.shape))
        out = np.empty((x.shape[0], nc), dtype=np.float32)
        rc, secs = _timed(lib().ccdgpu_classify, self._ctx, x.ctypes.data, x.shape[0], out.ctypes.data)
        _check(rc)
        self.forest_seconds = secs
        return out

    def classify_rows(self, aux, rows_cap=None):
        """rfrawp float32 [n_rows][n_classes] of the rows of the last completed run, in the order
        fetch_batch_rows_into / fetch_rows give them, gathered and classified on the device
        (ccdgpu_classify_rows).  aux [total_pixels][5] float64: dem, aspect, slope, mpw, posidex.
        Rows without a model are NaN.  ``rows_cap`` (tests): the buffer's room instead of a size
        learned from the library."""
        nc = self._forest_dims()[1]
        a = np.ascontiguousarray(aux, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 5:
            raise ValueError('aux must be [total_pixels][5], got %r' % (a.shape,))
        n_pix = self._last.total_pixels
        if n_pix is not None and a.shape[0] != n_pix:
            raise ValueError('aux has %d pixels, the batch %d' % (a.shape[0], n_pix))
        nr = ctypes.c_int64(0)
        L = lib()
        cap = int(rows_cap) if rows_cap is not None else 2 * a.shape[0] + 64
        for _ in range(2):
            out = np.empty((cap, nc), dtype=np.float32)
            rc, secs = _timed(L.ccdgpu_classify_rows, self._ctx, a.ctypes.data, out.ctypes.data, cap, ctypes.byref(nr))
            if rc == 0:
                break
            if rows_cap is not None or rc != abi.E_INVAL or nr.value <= cap:
                self.forest_rows = nr.value
                _check(rc)
            cap = nr.value  # more rows than the first guess
        else:
            _check(rc)
        self.forest_seconds = secs
        self.forest_rows = nr.value
        return out[:nr.value]

    def train_forest(self, x, labels, edges, n_classes=None, **params):
        """Train a random forest on the device by the rule of include/ccdgpu.h (ccdgpu_forest_train) and
        return it as a ccdc.randomforest.Forest: x [n_rows][n_features] float64, labels [n_rows] in
        0 .. n_classes-1 (n_classes None: max(label) + 1), edges one increasing sequence per feature
        (``ccdc.randomforest.find_splits``), params the fields of ``train_params``.  The context's own
        forest (``set_forest``) is untouched; the kernel seconds are in ``train_seconds``.  A request
        the library refuses raises CcdGpuError with its message."""
        from ccdc.randomforest import Forest
        args, keep = _train_args(x, labels, edges, n_classes, params)  # (keep: alive over the call)
        L = lib()
        rc, secs = _timed(L.ccdgpu_forest_train, self._ctx, *args)
        _check(rc)
        self.train_seconds = secs
        nt, nn = ctypes.c_int32(0), ctypes.c_int32(0)
        _check(L.ccdgpu_trained_size(self._ctx, ctypes.byref(nt), ctypes.byref(nn)))
        nc = args[4]
        f = Forest(np.empty(nt.value, np.int32), np.empty(nn.value, np.int32), np.empty(nn.value, np.float64),
                   np.empty(nn.value, np.int32), np.empty(nn.value, np.int32), np.empty((nn.value, nc), np.float64), args[3])
        _check(L.ccdgpu_trained_fetch(self._ctx, ctypes.byref(f.struct())))
        # what the out-of-bag estimate and the importances need (Forest.save keeps them)
        f.counts = np.empty((nn.value, nc), np.int64)
        _check(L.ccdgpu_trained_counts(self._ctx, f.counts.ctypes.data, f.counts.size))
        p = keep[-1]
        f.seed, f.bootstrap = int(p.seed), bool(p.bootstrap)
        return f

    def find_splits(self, x, max_bins=32):
        """The bin edges of x [n_rows][n_features] float64 (finite values), found on the device by the
        position form of the rule in include/ccdgpu.h (ccdgpu_forest_find_splits): a list of increasing
        float64 arrays, one per feature, equal array by array to ``ccdc.randomforest.find_splits`` on the
        host.  The kernel seconds are in ``splits_seconds``.  A request the library's checks refuse (a
        non-finite value, max_bins outside 2 .. 64: ccdgpu_splits_check, run by the call before anything
        is launched) raises ValueError with the library's message; any other refusal raises CcdGpuError."""
        args, keep = _splits_args(x, max_bins)  # (keep: alive over the call)
        nf = args[2]
        edges = np.empty((nf, abi.TRAIN_MAX_EDGES), dtype=np.float64)
        n_edges = np.empty(nf, dtype=np.int32)
        rc, secs = _timed(lib().ccdgpu_forest_find_splits, self._ctx, *(args + (edges.ctypes.data, n_edges.ctypes.data)))
        if rc == abi.E_INVAL and last_error().startswith('splits: '):
            raise ValueError(last_error())
        _check(rc)
        self.splits_seconds = secs
        return [np.ascontiguousarray(edges[f, :n_edges[f]]) for f in range(nf)]

    def forest_oob(self, x, seed, first_row=0):
        """The out-of-bag walk of include/ccdgpu.h (ccdgpu_forest_oob) of x [n_rows][n_features] float64
        through the forest set: row i, with hash index first_row + i, is scored only by the trees whose
        bag under ``seed`` it is not in.  Returns (oob_raw float32 [n_rows][n_classes], n_oob int32
        [n_rows]: the trees that scored the row; 0: the row is all zeros); the kernel seconds are in
        ``oob_seconds``.  A request the library refuses raises CcdGpuError with its message."""
        nf, nc = self._forest_dims()
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != nf:
            raise ValueError('x must be [n_rows][%d], got %r' % (nf, x.shape))
        p = abi.OobParams()
        p.seed, p.first_row = int(seed), int(first_row)
        raw = np.empty((x.shape[0], nc), dtype=np.float32)
        n_oob = np.empty(x.shape[0], dtype=np.int32)
        rc, secs = _timed(lib().ccdgpu_forest_oob, self._ctx, x.ctypes.data, x.shape[0], ctypes.byref(p), raw.ctypes.data,
                          n_oob.ctypes.data)
        _check(rc)
        self.oob_seconds = secs
        return raw, n_oob

    def forest_permutation(self, x, labels, seed, perm_seed=0):
        """The out-of-bag permutation counts of include/ccdgpu.h (ccdgpu_forest_permutation) of the forest
        set over x [n_rows][n_features] float64 and labels [n_rows] in 0 .. n_classes-1, the whole
        training matrix in training order: per tree, over the rows out of its bag under ``seed``,
        (oob_rows [n_trees][n_classes], correct [n_trees][n_classes], lost and gained
        [n_trees][n_features][n_classes]), all int64 -- the rows of each label, those the tree votes
        right, and the right votes lost and gained when a feature's column is shuffled by ``perm_seed``.
        The kernel seconds are in ``permutation_seconds``.  A request the library refuses raises
        CcdGpuError with its message."""
        nf, nc = self._forest_dims()
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != nf:
            raise ValueError('x must be [n_rows][%d], got %r' % (nf, x.shape))
        y = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if y.shape[0] != x.shape[0]:
            raise ValueError('labels must be [%d], got %r' % (x.shape[0], y.shape))
        nt = self._forest_trees
        p = abi.PermutationParams()
        p.seed, p.perm_seed = int(seed), int(perm_seed)
        oob_rows, correct = np.empty((nt, nc), np.int64), np.empty((nt, nc), np.int64)
        lost, gained = np.empty((nt, nf, nc), np.int64), np.empty((nt, nf, nc), np.int64)
        rc, secs = _timed(lib().ccdgpu_forest_permutation, self._ctx, x.ctypes.data, y.ctypes.data, x.shape[0], ctypes.byref(p),
                          oob_rows.ctypes.data, correct.ctypes.data, lost.ctypes.data, gained.ctypes.data)
        _check(rc)
        self.permutation_seconds = secs
        return oob_rows, correct, lost, gained

    # prediction of band values from segment models -----------------------------------------------
    def coefficient_matrix(self, dates, avg_days_yr=365.2425):
        """The device's basis of ``dates`` (ordinals): float64 [n_dates][7] = t, cos/sin of 1, 2
        and 3 cycles per year -- the reference's coefficient_matrix(dates, avg_days_yr, 8)
        (ccdgpu_coefficient_matrix)."""
        d = _predict_dates(dates)
        out = np.empty((d.shape[0], 7), dtype=np.float64)
        _check(lib().ccdgpu_coefficient_matrix(self._ctx, d.shape[0], d.ctypes.data, float(avg_days_yr), out.ctypes.data))
        return out

    def predict(self, row_offsets, rows, dates, avg_days_yr=365.2425, cover='span', dtype='float32', seg_index=True,
                out=None):
        """Band values of a host table of segment rows at ``dates`` (ccdgpu_predict; the rule is in
        include/ccdgpu.h): pixel p has rows[row_offsets[p]:row_offsets[p + 1]] (abi.ROW_DTYPE).
        Returns (values [7][n_pix][n_dates] float32 or int16, seg_index int32 [n_pix][n_dates] or
        None); the kernel seconds are in ``predict_seconds``.  ``out`` / ``seg_index`` may be arrays of
        those shapes and types to fill instead of new ones -- the call is the copy of its output, and
        page-locked arrays (``pinned_empty``), reused, receive it by DMA at the link's speed.
        Arguments that fail ccdgpu_predict_check raise CcdGpuError (E_INVAL) with the library's message."""
        off, r = _row_table(row_offsets, rows)
        d = _predict_dates(dates)
        cover, dtype = _predict_modes(cover, dtype)
        n_pix = off.shape[0] - 1
        out, idx = _predict_buffers(out, seg_index, n_pix, d.shape[0], dtype)
        rc, secs = _timed(lib().ccdgpu_predict, self._ctx, n_pix, off.ctypes.data, r.ctypes.data, d.shape[0], d.ctypes.data,
                          float(avg_days_yr), cover, dtype, out.ctypes.data, _ptr(idx))
        _check(rc)
        self.predict_seconds = secs
        return out, idx

    def predict_rows(self, chip, dates, avg_days_yr=365.2425, cover='span', dtype='float32', seg_index=True, out=None):
        """``predict`` for the pixels of chip ``chip`` of the last completed run, from its segments
        on the device (ccdgpu_predict_rows): the bytes ``predict`` gives on ``fetch_rows(chip, ..)``.
        ``out`` / ``seg_index`` as for ``predict``."""
        d = _predict_dates(dates)
        cover, dtype = _predict_modes(cover, dtype)
        chip = int(chip)

        def call(out, idx):
            rc, secs = _timed(lib().ccdgpu_predict_rows, self._ctx, chip, d.shape[0], d.ctypes.data, float(avg_days_yr),
                              cover, dtype, _ptr(out), _ptr(idx))
            _check(rc)
            return secs

        n_pix = self._chip_pixels(chip, lambda: call(None, None), 'no completed run to predict from')
        out, idx = _predict_buffers(out, seg_index, n_pix, d.shape[0], dtype)
        self.predict_seconds = call(out, idx)
        return out, idx

    # annual change and land-cover product rasters from segments ------------------------------------
    def products(self, row_offsets, rows, dates, rfrawp=None, params=None, want=None, out=None, **kw):
        """Product rasters of a host table of segment rows at ``dates`` (ccdgpu_products; the rule is in
        include/ccdgpu.h): pixel p has rows[row_offsets[p]:row_offsets[p + 1]] (abi.ROW_DTYPE), rfrawp
        float32 [n_rows][n_classes] is row-aligned with them (None: no cover products).  ``params`` an
        abi.ProductParams, or the keywords of ``product_params`` (bot, mag_bands, cover, n_classes,
        labels).  Returns {name: array [n_dates][n_pix]} for the names in ``want`` (abi.PRODUCTS; None:
        the change products, and the cover products when there is an rfrawp); ``out`` may map names to
        arrays to fill instead of new ones (page-locked ones, ``pinned_empty``, receive them by DMA).
        The kernel seconds are in ``products_seconds``.  Arguments that fail ccdgpu_products_check
        raise CcdGpuError (E_INVAL) with the library's message."""
        off, r = _row_table(row_offsets, rows)
        d = _predict_dates(dates)
        p = product_params(**kw) if params is None else params
        rf = _rfrawp(rfrawp, r.shape[0], p)
        want, arrays, ptrs = _product_request(want, out, off.shape[0] - 1, d.shape[0], rf is not None)
        rc, secs = _timed(lib().ccdgpu_products, self._ctx, off.shape[0] - 1, off.ctypes.data, r.ctypes.data, _ptr(rf),
                          d.shape[0], d.ctypes.data, ctypes.byref(p), ctypes.byref(ptrs))
        _check(rc)
        self.products_seconds = secs
        return arrays

    def products_rows(self, chip, dates, rfrawp=None, params=None, want=None, out=None, **kw):
        """``products`` for the pixels of chip ``chip`` of the last completed run, from its segments on
        the device (ccdgpu_products_rows): the bytes ``products`` gives on ``fetch_rows(chip, ..)``.
        rfrawp: that chip's rows of ``classify_rows``, in ``fetch_rows`` order (None: no cover
        products); its row count is checked by the library's offsets, so pass exactly the chip's."""
        d = _predict_dates(dates)
        p = product_params(**kw) if params is None else params
        chip = int(chip)
        rf = None
        if rfrawp is not None:
            rf = np.ascontiguousarray(rfrawp, dtype=np.float32)
            rf = _rfrawp(rf, rf.shape[0], p)

        def call(rf, n_dates, dates, ptrs):
            rc, secs = _timed(lib().ccdgpu_products_rows, self._ctx, chip, _ptr(rf), n_dates, dates, ctypes.byref(p),
                              ctypes.byref(ptrs))
            _check(rc)
            return secs

        probe = abi.Products()
        probe.sctime = 1
        n_pix = self._chip_pixels(chip, lambda: call(None, 0, None, probe), 'no completed run to make products from')
        want, arrays, ptrs = _product_request(want, out, n_pix, d.shape[0], rf is not None)
        if rf is not None:  # the chip's rows: a row per segment, one for a pixel without any
            n_rows = self.chip_row_count(chip)
            if rf.shape[0] != n_rows:
                raise ValueError('rfrawp has %d rows, chip %d has %d' % (rf.shape[0], chip, n_rows))
        self.products_seconds = call(rf, d.shape[0], d.ctypes.data, ptrs)
        return arrays

    def chip_row_count(self, chip):
        """Rows ``fetch_rows`` gives for chip ``chip`` of the last completed run (a row per segment, one
        for a pixel without any): the chip's share of ``classify_rows``' rows, chips in order
        (ccdgpu_chip_row_count; no device work)."""
        n = ctypes.c_int64(0)
        _check(lib().ccdgpu_chip_row_count(self._ctx, int(chip), ctypes.byref(n)))
        return n.value

    def diag_counters(self):
        buf = (ctypes.c_uint64 * 48)()
        _check(lib().ccdgpu_diag_counters(self._ctx, buf, 48))
        return list(buf)

    def stats(self):
        s = abi.Stats()
        _check(lib().ccdgpu_last_stats(self._ctx, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in abi.Stats._fields_}


class _Pinned(object):
    """Owner of one ccdgpu_host_alloc block (freed when the last array view goes away)."""
    def __init__(self, nbytes):
        self.ptr = ctypes.c_void_p()
        _check(lib().ccdgpu_host_alloc(int(nbytes), ctypes.byref(self.ptr)))
        self.nbytes = int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                lib().ccdgpu_host_free(self.ptr)
        except Exception:
            pass


def batch_storage(max_chips, max_pix, max_obs, pinned=True):
    """Reusable buffers for ChipBatch(..., storage=...): room for ``max_chips`` chips of up to
    ``max_pix`` pixels x ``max_obs`` observations."""
    alloc = _allocator(pinned)
    n = int(max_chips) * int(max_pix) * int(max_obs)
    return (alloc((int(max_chips) * int(max_obs),), np.int64), alloc((7 * n,), np.int16), alloc((n,), np.uint16))


class RowsBuffers(object):
    """Reusable (pinned) landing buffers of Context.fetch_batch_rows_into: row offsets, rows
    (abi.ROW_DTYPE) and mask words; grown on demand, 25 % headroom."""

    def __init__(self, pinned=True, rows_per_pixel=2.0):
        self.pinned = pinned
        self.rows_per_pixel = float(rows_per_pixel)  # rows room of a batch chain (run_slot_begin_rows)
        # rows a batch chain copies back per pixel: learned from the batches seen (1.25 x the
        # highest rate, at most rows_per_pixel), so the copy is not the whole room -- a tile of
        # ~1 row per pixel copies ~1.25 instead of 2 rows' bytes per pixel; a batch with more
        # rows than that takes the rows-overflow path once and raises the rate
        self.copy_per_pixel = None
        self.max_rate = 0.0
        self.offsets = np.zeros(0, np.int64)
        self.rows = np.zeros(0, abi.ROW_DTYPE)
        self.mask = np.zeros(0, np.uint32)

    def _grow(self, arr, n, dtype):
        if arr.size >= n:
            return arr
        n = int(n * 1.25) + 64
        return _allocator(self.pinned)((n,), dtype)

    def ensure(self, n_offsets, n_rows, n_words):
        self.offsets = self._grow(self.offsets, n_offsets, np.int64)
        self.rows = self._grow(self.rows, n_rows, abi.ROW_DTYPE)
        self.mask = self._grow(self.mask, n_words, np.uint32)

    def reserve(self, n_pix, words):
        """Grow the buffers for a batch chain of ``n_pix`` pixels with ``words`` mask words each
        (run_slot_begin_rows): returns (the rows room, the rows the chain copies back -- the learned
        rate's, within the room)."""
        self.ensure(n_pix + 1, int(self.rows_per_pixel * n_pix) + 64, n_pix * words)
        rate = self.copy_per_pixel if self.copy_per_pixel is not None else self.rows_per_pixel
        return self.rows.size, min(self.rows.size, int(rate * n_pix) + 64)

    def learn(self, n_rows, n_pix, cap):
        """Learn from a finished batch chain of ``n_pix`` pixels that had ``n_rows`` rows and copied
        ``cap`` back: ``max_rate`` and ``copy_per_pixel`` follow the rate seen; more rows than the copy
        held also raise ``rows_per_pixel``, and the answer is True: the rows must be fetched."""
        if n_rows > 0:
            self.max_rate = max(self.max_rate, n_rows / max(1, n_pix))
            self.copy_per_pixel = min(self.rows_per_pixel, 1.25 * self.max_rate)
        if n_rows <= cap:
            return False
        self.rows_per_pixel = max(self.rows_per_pixel, 1.25 * n_rows / max(1, n_pix))
        self.copy_per_pixel = min(self.rows_per_pixel, 1.25 * self.max_rate)
        return True


def pinned_empty(shape, dtype):
    """numpy array in pinned (page-locked) host memory: uploads from it are asynchronous."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    owner = _Pinned(n)
    buf = (ctypes.c_char * max(n, 1)).from_address(owner.ptr.value)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    return _PinnedArray(arr, owner)


class _PinnedArray(np.ndarray):
    """ndarray view whose base keeps the pinned allocation alive."""
    def __new__(cls, arr, owner):
        obj = np.asarray(arr).view(cls)
        obj._pinned_owner = owner
        return obj

    def __array_finalize__(self, obj):
        if obj is not None:
            self._pinned_owner = getattr(obj, '_pinned_owner', None)


_default_ctx = {}


def default_context(device=None):
    """Per-thread default context on ``device`` (HIP_VISIBLE_DEVICES-relative, default 0)."""
    if device is None:
        device = int(os.environ.get('CCDGPU_DEVICE', '0'))
    key = (threading.get_ident(), device)
    ctx = _default_ctx.get(key)
    if ctx is None:
        ctx = Context(device)
        _default_ctx[key] = ctx
    return ctx
