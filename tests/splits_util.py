"""The bin-edge rule in the position form include/ccdgpu.h states it in (what ccd_splits.hip
computes), in numpy, and the columns the splits tests share.  ``find_splits`` here must equal
ccdc.randomforest.find_splits array by array."""
import numpy as np


def column_edges(column, max_bins):
    """The edges of one column by the header's position form."""
    s = np.sort(np.asarray(column, dtype=np.float64) + 0.0)  # key: -0.0 + 0.0 is +0.0
    n = s.shape[0]
    p = (np.flatnonzero(s[1:] != s[:-1]) + 1).tolist()  # the boundaries, ascending
    if len(p) <= max_bins - 1:
        taken = p
    else:
        stride = float(n) / float(max_bins)
        target = stride
        succ = p[1:] + [n]
        taken = []
        for pi, pn in zip(p, succ):
            if abs(float(pi) - target) < abs(float(pn) - target):
                taken.append(pi)
                target += stride
    out = []
    with np.errstate(over='ignore'):
        prev = None
        for pi in taken:
            mid = (s[pi - 1] + s[pi]) / 2.0
            if prev is None or mid > prev:
                out.append(mid)
            prev = mid
    return np.asarray(out, dtype=np.float64)


def find_splits(matrix, max_bins=32):
    x = np.asarray(matrix, dtype=np.float64)
    return [column_edges(x[:, f], max_bins) for f in range(x.shape[1])]


def same(a, b):
    """Two lists of edge arrays are equal array by array (dtype, shape, every value; inf equals inf)."""
    return len(a) == len(b) and all(u.dtype == v.dtype == np.float64 and u.shape == v.shape and np.array_equal(u, v)
                                    for u, v in zip(a, b))


def host(matrix, max_bins):
    """ccdc.randomforest.find_splits on the host (an overflowing midpoint warns in numpy: silenced)."""
    from ccdc import randomforest
    with np.errstate(over='ignore'):
        return randomforest.find_splits(matrix, max_bins)


def _distinct(rng, n, k):
    """n values over exactly k distinct normal draws, every one present."""
    v = np.unique(rng.normal(size=4 * k + 8))[:k]
    c = np.concatenate([v, rng.choice(v, size=n - k)])
    rng.shuffle(c)
    return c


def kinds(n, max_bins, seed=0):
    """{name: column of n values} -- the column kinds of the issue, n >= 2 * max_bins + 2."""
    rng = np.random.default_rng(seed)
    tiny = 5e-324
    out = {}
    out['ordinary'] = rng.normal(size=n)
    out['constant'] = np.full(n, 1.25)
    for k in (max_bins - 1, max_bins, max_bins + 1):  # the switch between the two branches
        out['distinct_%+d' % (k - max_bins)] = _distinct(rng, n, k)
    out['skew_of_ties'] = np.floor(40.0 * rng.exponential(size=n))
    signs = rng.integers(-3, 4, size=n).astype(np.float64)
    signs[signs == 0] = np.where(rng.random(int((signs == 0).sum())) < 0.5, -0.0, 0.0)
    signs[:2] = (-0.0, 0.0)  # both zeros present
    out['both_signs_and_zeros'] = signs
    out['denormals'] = rng.integers(-200, 200, size=n).astype(np.float64) * tiny
    near = np.full(n, 1.0)
    for i in range(1, 6):
        near[i::6] = np.nextafter(near[i - 1], 2.0)  # 1.0 and its next five neighbours: a midpoint repeats
    out['neighbouring_doubles'] = near
    huge = rng.choice(np.array([-1.7e308, -1.6e308, 0.0, 1.0, 1.6e308, 1.7e308]), size=n)
    huge[:6] = (-1.7e308, -1.6e308, 0.0, 1.0, 1.6e308, 1.7e308)
    out['huge_both_sides'] = huge  # (+-1.7e308 + +-1.6e308) overflows: an edge is inf on either side
    bits = rng.integers(0, 1 << 63, size=2 * n, dtype=np.int64).astype(np.uint64) | \
        (rng.integers(0, 2, size=2 * n).astype(np.uint64) << np.uint64(63))
    vals = bits.view(np.float64)
    vals = vals[np.isfinite(vals)][:n]
    assert vals.shape[0] == n
    out['random_bit_patterns'] = vals  # every radix pass moves keys
    base = np.float64(1.5).view(np.uint64)
    # (positive values whose exponents' high bits differ and nothing else: seven radix passes are skipped)
    top = np.uint64(0x2000000000000000) + (rng.integers(0, 4, size=n).astype(np.uint64) << np.uint64(60))
    out['top_byte_only'] = ((base & np.uint64(0x00FFFFFFFFFFFFFF)) | top).view(np.float64)
    out['bottom_byte_only'] = (base + rng.integers(0, 256, size=n).astype(np.uint64)).view(np.float64)
    for name, c in out.items():
        assert c.shape == (n,) and np.all(np.isfinite(c)), name
    return out


HAND = [0.0] * 10 + [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]  # at max_bins 4 one value spans several targets
