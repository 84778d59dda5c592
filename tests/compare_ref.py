"""The yardstick of erpl_mc_compare in plain NumPy: the two-sample statistics (Kolmogorov-Smirnov, Mann-Whitney,
Cramer-von Mises, the energy statistic) of two samples under a given labelling, the integers exactly (Python ints), U of
Cramer-von Mises as an exact rational and the energy statistic in np.longdouble, each next to its plain float64 evaluation
(the figure the device's error is measured against).  The labels of a permutation are restated here from the contract of
include/erpl_mc.h through philox_ref; nothing is shared with the library."""
from fractions import Fraction

import numpy as np

import philox_ref as PR

LD = np.longdouble


def labels(seed, permutation, m_a, m_b):
    """Side A (True) of permutation `permutation`: the m_a pooled members with the smallest (key, i) pairs, the key of member
    i being draw i of replicate `permutation`: Philox pair i >> 1, word A if i is even, else B."""
    seed, n = int(seed), int(m_a) + int(m_b)
    i = np.arange(n, dtype=np.uint64)
    j = i >> np.uint64(1)
    o = PR.philox4x32_10((j & PR.MASK, j >> PR.S32, permutation, 0), (seed & 0xFFFFFFFF, seed >> 32))
    key = np.where((i & np.uint64(1)) == 0, o[0] | (o[1] << PR.S32), o[2] | (o[3] << PR.S32))
    order = np.lexsort((i, key))   # by key, then by index
    out = np.zeros(n, dtype=bool)
    out[order[:int(m_a)]] = True
    return out


def identity(m_a, m_b):
    return np.arange(m_a + m_b) < m_a


def quantile(x, q):
    """The library's quantile: pos = q (m - 1), order_lo + (order_hi - order_lo) (pos - floor(pos))."""
    s = np.sort(np.asarray(x, dtype=np.float64))
    m = len(s)
    pos = q * float(m - 1)
    lo = min(int(np.floor(pos)), m - 1)
    hi = min(lo + 1, m - 1)
    return s[lo] + (s[hi] - s[lo]) * (pos - np.floor(pos))


class Ranked:
    """The pooled sorted order of one row: what does not depend on the labelling."""

    def __init__(self, z):
        z = np.asarray(z, dtype=np.float64) + 0.0        # -0.0 ties with +0.0
        self.n = len(z)
        self.order = np.argsort(z, kind="stable")        # (value, pooled index) ascending
        self.zs = z[self.order]
        new = np.r_[True, self.zs[1:] != self.zs[:-1]]
        self.end = np.r_[new[1:], True]
        cls = np.cumsum(new) - 1
        first = np.flatnonzero(new)[cls]
        last = np.flatnonzero(self.end)[cls]
        self.r2 = (first + last + 2).astype(np.int64)    # the doubled 1-based mid-rank


def rank_stats(rk, lab):
    """K, its location, value and sign, 2 U_A, T (longdouble, from the exact rational) and T in plain float64."""
    la = np.asarray(lab, dtype=bool)[rk.order]
    n, m_a = rk.n, int(la.sum())
    m_b = n - m_a
    ca = np.cumsum(la).astype(np.int64)
    cb = np.arange(1, n + 1, dtype=np.int64) - ca
    v = m_b * ca - m_a * cb
    ends = np.flatnonzero(rk.end)
    av = np.abs(v[ends])
    k = int(av.max())
    at = int(ends[np.argmax(av)])                        # argmax: the first
    u2 = int(rk.r2[la].sum()) - m_a * (m_a + 1)
    d = rk.r2 - 2 * np.where(la, ca, cb)
    if n < 2 ** 20:                                      # d^2 < 2^42, the sums below 2^62: exact in int64
        sa, sb = int(np.dot(d[la], d[la])), int(np.dot(d[~la], d[~la]))
    else:
        sa, sb = sum(int(x) * int(x) for x in d[la]), sum(int(x) * int(x) for x in d[~la])
    t = Fraction(m_a * sa + m_b * sb, 4 * m_a * m_b * n) - Fraction(4 * m_a * m_b - 1, 6 * n)
    t_ld = LD(float(t)) + LD(float(t - Fraction(float(t))))   # head + tail of the exact rational
    r = rk.r2 / 2.0
    u64 = m_a * np.sum((r[la] - ca[la]) ** 2) + m_b * np.sum((r[~la] - cb[~la]) ** 2)
    t64 = u64 / (float(m_a) * m_b * n) - (4.0 * m_a * m_b - 1.0) / (6.0 * n)
    return {"K": k, "at": at, "value": float(rk.zs[at]), "sign": int(np.sign(v[at])), "U2": u2, "T": t_ld, "T64": float(t64),
            "D": k / (float(m_a) * float(m_b)), "mw": abs(u2 - m_a * m_b)}


class Cloud:
    """The pooled distance matrix of the impact points, in longdouble and in float64."""

    def __init__(self, x, y, exact=True):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
        self.d64 = np.sqrt(dx * dx + dy * dy)
        if exact:
            xl, yl = x.astype(LD), y.astype(LD)
            dx, dy = xl[:, None] - xl[None, :], yl[:, None] - yl[None, :]
            self.d = np.sqrt(dx * dx + dy * dy)
            self.row = self.d.sum(axis=1)


def energy_f64_all(cl, labs):
    """E of every labelling of `labs` in plain float64, all at once (one matrix product): what decides a test case."""
    f = np.stack(labs, axis=1).astype(np.float64)          # [N, Q]
    m_a = f[:, 0].sum()
    m_b = f.shape[0] - m_a
    to_a = cl.d64 @ f
    s_aa, s_ab = (f * to_a).sum(axis=0), ((1.0 - f) * to_a).sum(axis=0)
    s_bb = ((1.0 - f) * (cl.d64.sum(axis=1)[:, None] - to_a)).sum(axis=0)
    return 2.0 * s_ab / (m_a * m_b) - s_aa / (m_a * m_a) - s_bb / (m_b * m_b)


def energy_stats(cl, lab):
    """E = 2 d_ab - d_aa - d_bb with the three mean distances (longdouble) and E in plain float64."""
    la = np.asarray(lab, dtype=bool)
    m_a, m_b = int(la.sum()), int((~la).sum())
    ra = cl.d[:, la].sum(axis=1)                         # to side A, from every member
    s_aa, s_ab = ra[la].sum(), ra[~la].sum()
    s_bb = (cl.row[~la] - ra[~la]).sum()
    d_aa, d_ab, d_bb = s_aa / (LD(m_a) * m_a), s_ab / (LD(m_a) * m_b), s_bb / (LD(m_b) * m_b)
    f = la.astype(np.float64)
    g = 1.0 - f
    e64 = 2.0 * (f @ cl.d64 @ g) / (float(m_a) * m_b) - (f @ cl.d64 @ f) / (float(m_a) * m_a) - (g @ cl.d64 @ g) / (float(m_b) * m_b)
    return {"E": LD(2) * d_ab - d_aa - d_bb, "d_aa": d_aa, "d_ab": d_ab, "d_bb": d_bb, "E64": float(e64)}


def null_summary(values, observed, level):
    """exceed, p, mean and np.quantile(level) of the null values of one test."""
    v = np.asarray(values)
    exceed = int(np.sum(v >= observed))
    return {"exceed": exceed, "p": (exceed + 1) / (len(v) + 1), "mean": float(np.mean(v.astype(np.float64))),
            "hi": float(np.quantile(v.astype(np.float64), level))}


def compare(a_rows, b_rows, a_xy=None, b_xy=None, permutations=0, seed=0, labeller=labels):
    """The whole comparison of two populations given as lists of value rows ([R][m_a], [R][m_b]) and optional (x, y) pairs:
    per row the observed statistics and the list of the null ones, and the same for the energy statistic."""
    m_a, m_b = len(a_rows[0]), len(b_rows[0])
    labs = [identity(m_a, m_b)] + [labeller(seed, p, m_a, m_b) for p in range(permutations)]
    out = {"m_a": m_a, "m_b": m_b, "rows": [], "labels": labs}
    for a, b in zip(a_rows, b_rows):
        rk = Ranked(np.r_[a, b])
        out["rows"].append([rank_stats(rk, lab) for lab in labs])
    if a_xy is not None:
        cl = Cloud(np.r_[a_xy[0], b_xy[0]], np.r_[a_xy[1], b_xy[1]])
        out["energy"] = [energy_stats(cl, lab) for lab in labs]
    return out
