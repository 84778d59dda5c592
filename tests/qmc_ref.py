"""The contract of erpl_mc_qmc in NumPy (vectorised uint64): the Joe-Kuo direction numbers expanded from SciPy's own copy of
the table by the recurrence, the binary-order Sobol' point, the lazy nested uniform scramble, the probability.  Philox comes
from philox_ref, the jitter and the pad rows from design_ref.  Written from the contract in include/erpl_mc.h; shares no code
with the library."""
import functools
import os

import numpy as np

import design_ref
import philox_ref
from philox_ref import MASK

RAW, OWEN = 0, 1
MAX_DIMS = 1024
TAG = 4


@functools.lru_cache(maxsize=None)
def direction_numbers(dims=MAX_DIMS):
    """V[dims][32] (uint64 holding 32-bit words): V[d][j] = m_(j+1) 2^(31 - j)."""
    import scipy.stats
    data = np.load(os.path.join(os.path.dirname(scipy.stats.__file__), "_sobol_direction_numbers.npz"))
    poly, vinit = data["poly"], data["vinit"]
    V = np.zeros((dims, 32), dtype=np.uint64)
    V[0] = [1 << (31 - j) for j in range(32)]
    for d in range(1, dims):
        p = int(poly[d])
        s = p.bit_length() - 1
        a = [(p >> (s - k)) & 1 for k in range(1, s)]          # a_1 .. a_(s-1)
        m = [int(v) for v in vinit[d, :s]]
        for k in range(s, 32):
            new = m[k - s] ^ (m[k - s] << s)
            for t in range(1, s):
                if a[t - 1]:
                    new ^= m[k - t] << t
            m.append(new)
        V[d] = [m[j] << (31 - j) for j in range(32)]
    return V


def raw_points(d, ell):
    """x of the local indices `ell` on dimension d: the XOR of V[d][j] over the set bits j of ell."""
    V = direction_numbers()
    ell = np.asarray(ell, dtype=np.uint64)
    x = np.zeros(ell.shape, dtype=np.uint64)
    for j in range(31):
        x ^= np.where((ell >> np.uint64(j)) & np.uint64(1) == 1, V[d, j], np.uint64(0))
    return x


def scramble_keys(seed, row, replicate):
    o = philox_ref.philox4x32_10((row, 0, replicate, TAG), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    return int(o[0][0]), int(o[1][0])


def owen(x, k0, k1):
    """Bit k from the top of x flipped by a hash of the k bits above it (of the unscrambled x) under a sentinel bit."""
    x = np.asarray(x, dtype=np.uint64)
    flips = np.zeros(x.shape, dtype=np.uint64)
    for k in range(32):
        prefix = (x >> np.uint64(32 - k)) if k else np.zeros(x.shape, dtype=np.uint64)
        s = np.uint64(1 << k) | prefix
        h = design_ref.fmix32(design_ref.fmix32((s + np.uint64(k0)) & MASK) ^ np.uint64(k1))
        flips |= (h >> np.uint64(31)) << np.uint64(31 - k)
    return x ^ flips


def inverse_gray(i):
    i = np.array(i, dtype=np.uint64)
    shift = 1
    while shift < 64:
        i ^= i >> np.uint64(shift)
        shift *= 2
    return i


def qmc(seed, rows, n, block=0, first=0, count=None, first_row=0, dims=None, scramble=OWEN, pad=design_ref.RANDOM):
    """p of the columns first .. first + count - 1 of the rows first_row .. first_row + rows - 1: float64 [rows, count]."""
    m = n if block == 0 else block
    assert 1 <= m <= n and n % m == 0
    count = n - first if count is None else count
    if dims is None:
        dims = [first_row + r if first_row + r < MAX_DIMS else -1 for r in range(rows)]
    cols = np.arange(first, first + count, dtype=np.int64)
    rep, ell = cols // m, cols % m
    p = np.empty((rows, count))
    for r in range(rows):
        g = first_row + r
        if dims[r] < 0:
            p[r] = design_ref.design(seed, pad, 1, n, block, first, count, g)[0][0]
            continue
        x = raw_points(dims[r], ell)
        if scramble == RAW:
            p[r] = (x.astype(np.float64) + 0.5) * 2.0 ** -32
            continue
        xs = np.empty_like(x)
        for q in np.unique(rep):
            sel = rep == q
            xs[sel] = owen(x[sel], *scramble_keys(seed, g, int(q)))
        top = xs.astype(np.float64) + 1.0
        s = xs.astype(np.float64) + design_ref.jitter(seed, g, cols)
        s = np.where(s >= top, np.nextafter(top, 0.0), s)
        p[r] = s * 2.0 ** -32
    return p
