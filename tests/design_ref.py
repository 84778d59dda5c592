"""The design contract of erpl_mc_design in NumPy (vectorised uint64), on top of philox_ref: round keys, the cycle-walking
Feistel permutation, the jitter and the probability p.  Written from the contract in include/erpl_mc.h and checked against
its known answers by test_design_abi.py; shares no code with the library.  Normal rows are scipy.special.ndtri of p."""
import numpy as np

import philox_ref
from philox_ref import MASK, S32

RANDOM, LHS, LHS_CENTRED = 0, 1, 2
UNIFORM, NORMAL = 0, 1


def _key(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, seed >> 32


def round_keys(seed, row, replicate=0):
    """The six 32-bit round keys of (row, replicate): counters (row, 0, replicate, 2) and (row, 1, replicate, 2)."""
    a = philox_ref.philox4x32_10((row, 0, replicate, 2), _key(seed))
    b = philox_ref.philox4x32_10((row, 1, replicate, 2), _key(seed))
    return [int(a[0][0]), int(a[1][0]), int(a[2][0]), int(a[3][0]), int(b[0][0]), int(b[1][0])]


def fmix32(x):
    """The MurmurHash3 finaliser on uint64 arrays holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & MASK
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & MASK
    return x ^ (x >> np.uint64(16))


def half_bits(m):
    b = 1
    while 4 ** b < m:
        b += 1
    return b


def perm(keys, m, ell):
    """pi(ell) over [0, m): six Feistel rounds on 2 b bits, walked until the value is below m."""
    b = np.uint64(half_bits(m))
    mask = np.uint64((1 << int(b)) - 1)
    x = np.array(ell, dtype=np.uint64, ndmin=1)
    todo = np.ones(x.shape, dtype=bool)
    for _ in range(4096):
        left, right = x[todo] >> b, x[todo] & mask
        for k in keys:
            left, right = right, left ^ (fmix32((right + np.uint64(k)) & MASK) & mask)
        x[todo] = (left << b) | right
        todo = x >= np.uint64(m)
        if not todo.any():
            return x.astype(np.int64)
    raise AssertionError("the walk did not end")


def jitter(seed, row, cols):
    """u of the GLOBAL columns `cols` of `row`: counter (j lo, j hi, row, 1), j = col >> 1, in (0, 1)."""
    i = np.asarray(cols, dtype=np.uint64)
    j = i >> np.uint64(1)
    o = philox_ref.philox4x32_10((j & MASK, j >> S32, row, 1), _key(seed))
    draw = np.where((i & np.uint64(1)) == 0, o[0] | (o[1] << S32), o[2] | (o[3] << S32))
    return ((draw >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def design(seed, kind, rows, n, block=0, first=0, count=None, first_row=0):
    """(p, pi) of columns first .. first + count - 1 of the rows first_row .. first_row + rows - 1: float64 and int64
    [rows, count].  pi is the stratum within the replicate (-1 for RANDOM)."""
    m = n if block == 0 else block
    assert 1 <= m <= n and n % m == 0
    count = n - first if count is None else count
    cols = np.arange(first, first + count, dtype=np.int64)
    rep, ell = cols // m, cols % m
    p = np.empty((rows, count))
    pi = np.full((rows, count), -1, dtype=np.int64)
    for r in range(rows):
        g = first_row + r
        u = jitter(seed, g, cols)
        if kind == RANDOM:
            p[r] = u
            continue
        for q in np.unique(rep):
            sel = rep == q
            pi[r, sel] = perm(round_keys(seed, g, int(q)), m, ell[sel])
        if kind == LHS_CENTRED:
            p[r] = (pi[r] + 0.5) / m
        else:
            s = pi[r].astype(np.float64) + u
            top = pi[r].astype(np.float64) + 1.0
            s = np.where(s >= top, np.nextafter(top, 0.0), s)
            p[r] = s / m
    return p, pi
