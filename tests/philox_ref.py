"""The tests' own Philox4x32-10 and the draw recipe of erpl_mc_bootstrap in NumPy (vectorised uint64): the yardstick of
erpl_mc_bootstrap_indices and of the replicates the device draws.  Written from the paper (Salmon, Moraes, Dror, Shaw,
SC 2011) and checked against the Random123 known answers by test_bootstrap_abi.py; shares no code with the library."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two 32-bit ints.  Returns the four output words (uint64 arrays
    holding 32-bit values)."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]   # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def mulhi64(u, m):
    """(u * m) >> 64 for uint64 arrays u and an int 0 < m < 2^32, in 32-bit limbs."""
    m = np.uint64(m)
    lo, hi = (u & MASK) * m, (u >> S32) * m
    return (hi + (lo >> S32)) >> S32


def indices(seed, replicate, m, first=0, count=None):
    """Dense indices of the draws first .. first + count - 1 of replicate `replicate` (int64 array)."""
    seed, m = int(seed), int(m)
    count = m - first if count is None else count
    t = np.arange(first, first + count, dtype=np.uint64)
    j = t >> np.uint64(1)
    o = philox4x32_10((j & MASK, j >> S32, replicate, 0), (seed & 0xFFFFFFFF, seed >> 32))
    a, b = o[0] | (o[1] << S32), o[2] | (o[3] << S32)
    u = np.where((t & np.uint64(1)) == 0, a, b)
    return mulhi64(u, m).astype(np.int64)
