"""The tests' own given-data sensitivity measures (NumPy / SciPy), sharing no code with the library.

Population: mask byte 0 and every factor and every row finite, in sample order; m members.
Classes: r = scipy.stats.rankdata (average ranks; -0.0 == 0.0), class = ((2 r - 1) K) // (2 m) in integers.
Tables: np.bincount.  With n_c the row sums, col_h the column sums, cum the running sums over h, in integers:
  delta_num = sum |m T - n_c col_h|           delta = float(delta_num) / ((2.0 m) m)
  ks_c      = float(max_h |m cumT - n_c cumcol|) / (float(m) float(n_c))    for n_c > 0;  ks_max, ks_median = np.median
  mi        = sum over T > 0 of (T / m) log((T m) / (n_c col_h)), factors taken as doubles, the terms added by math.fsum
              (correctly rounded: 64 equal terms of log(64) / 64 give log 64, which a running sum misses by 6 ulp)
Null: shift s_p = philox_ref.indices(seed, 0, m - 1, p, 1)[0] + 1; table p pairs xc[d] with yc[(d + s_p) % m];
  null_mean = the running sum over p ascending / P, null_hi = np.quantile(level), exceed = count(null >= estimate).
Variance share: the class sums in np.longdouble; B = sum n_c (mean_c - row_mean)^2, eta2 = B / row_ss,
  eta2_adj = 1 - (1 - eta2) (m - 1) / (m - k), f_stat = (B / (k - 1)) / ((row_ss - B) / (m - k))."""
import math

import numpy as np
from scipy.stats import rankdata

import philox_ref

MEASURES = ("delta", "ks_max", "ks_median", "mi")


def population(factors, ys, mask=None):
    keep = np.isfinite(factors).all(axis=0) & np.isfinite(ys).all(axis=0)
    if mask is not None:
        keep &= np.asarray(mask) == 0
    return keep


def class_of(x, K):
    """The class byte of every member of x (already the population)."""
    m = len(x)
    twice = np.rint(2.0 * rankdata(x, method="average") - 1.0).astype(np.int64)    # 2 r - 1: an integer
    return (twice * K) // (2 * m)


def table_of(xc, yc, M, H):
    return np.bincount(xc * H + yc, minlength=M * H).reshape(M, H).astype(np.int64)


def measures(T):
    """(delta_num, [delta, ks_max, ks_median, mi], classes_used, cells_used) of an int64 table."""
    m = int(T.sum())
    n_c, col = T.sum(axis=1), T.sum(axis=0)
    delta_num = int(np.abs(m * T - np.outer(n_c, col)).sum())
    delta = float(delta_num) / ((2.0 * float(m)) * float(m))
    used = n_c > 0
    D = np.abs(m * np.cumsum(T, axis=1) - n_c[:, None] * np.cumsum(col)[None, :]).max(axis=1)
    ks = D[used].astype(np.float64) / (float(m) * n_c[used].astype(np.float64))
    cs, hs = np.nonzero(T)                                     # c ascending, then h ascending
    t = T[cs, hs].astype(np.float64)
    terms = (t / float(m)) * np.log((t * float(m)) / (n_c[cs].astype(np.float64) * col[hs].astype(np.float64)))
    mi = math.fsum(terms.tolist())                             # the correctly rounded sum of the terms: no order to speak of
    return delta_num, [delta, float(ks.max()), float(np.median(ks)), mi], int(used.sum()), int((col > 0).sum())


def shifts_of(seed, m, P):
    return [int(philox_ref.indices(seed, 0, m - 1, p, 1)[0]) + 1 for p in range(P)]


def variance_share(xc, y, M):
    """Long double: (row_mean, row_ss, per class count / sum / sum|y| / mean / ss, eta2, eta2_adj, f_stat)."""
    L = np.longdouble
    y = y.astype(L)
    m = len(y)
    row_mean = y.sum() / L(m)
    row_ss = ((y - row_mean) ** 2).sum()
    count = np.bincount(xc, minlength=M).astype(np.int64)
    s, sa, mean, ss = np.zeros(M, L), np.zeros(M, L), np.full(M, np.nan, L), np.full(M, np.nan, L)
    for c in range(M):
        if count[c]:
            yc = y[xc == c]
            s[c], sa[c] = yc.sum(), np.abs(yc).sum()
            mean[c] = s[c] / L(count[c])
            ss[c] = ((yc - mean[c]) ** 2).sum()
    used = count > 0
    k = int(used.sum())
    B = (count[used].astype(L) * (mean[used] - row_mean) ** 2).sum()
    nan = L(np.nan)
    eta2 = eta2_adj = f_stat = nan
    if y.min() != y.max():
        if k < 2:
            eta2 = L(0)
        else:
            eta2 = B / row_ss
            if m > k:
                eta2_adj = 1 - (1 - eta2) * L(m - 1) / L(m - k)
                f_stat = (B / L(k - 1)) / ((row_ss - B) / L(m - k))
    return {"row_mean": row_mean, "row_ss": row_ss, "count": count, "sum": s, "sum_abs": sa, "mean": mean, "ss": ss, "B": B,
            "eta2": eta2, "eta2_adj": eta2_adj, "f_stat": f_stat}


def class_x(x, xc, M):
    """[M, 3]: x_lo, x_hi and x_median (the value of the middle member in sorted order, the lower of two) of every class."""
    out = np.full((M, 3), np.nan)
    for c in range(M):
        v = np.sort(x[xc == c], kind="stable")
        if len(v):
            out[c] = v[0], v[-1], v[(len(v) - 1) // 2]
    return out


def dependence(factors, ys, mask=None, classes=16, cells=16, shifts=200, level=0.95, seed=0):
    """factors [F, n] and ys [R, n] (the requested rows) -> the arrays of TrajectoryEngine.dependence, plus 'share': per
    (row, factor) the dict of variance_share (long double) and 'mi_cells' [R, F, 1 + P]: the non-empty cells of every table."""
    factors, ys = np.atleast_2d(np.asarray(factors, dtype=np.float64)), np.atleast_2d(np.asarray(ys, dtype=np.float64))
    F, R, M, H, P = len(factors), len(ys), classes, cells, shifts
    keep = population(factors, ys, mask)
    m = int(keep.sum())
    fx, fy = factors[:, keep], ys[:, keep]
    out = {"count": m, "classes_used": np.zeros((R, F), np.int64), "cells_used": np.zeros((R, F), np.int64),
           "delta_num": np.zeros((R, F), np.int64), "tables": np.zeros((R, F, M, H), np.int64),
           "class_stats": np.full((R, F, M, 6), np.nan), "null_values": np.full((R, F, 4, P), np.nan),
           "row_mean": np.full(R, np.nan), "row_ss": np.full(R, np.nan), "share": [[None] * F for _ in range(R)],
           "mi_cells": np.zeros((R, F, 1 + P), np.int64)}
    for key in ("eta2", "eta2_adj", "f_stat"):
        out[key] = np.full((R, F), np.nan)
    for key in MEASURES:
        out[key] = {"estimate": np.full((R, F), np.nan), "null_mean": np.full((R, F), np.nan),
                    "null_hi": np.full((R, F), np.nan), "exceed": np.zeros((R, F), np.int64)}
    out["class_stats"][..., 0] = 0.0
    if m == 0:
        return out
    xc = [class_of(fx[f], M) for f in range(F)]
    yc = [class_of(fy[j], H) for j in range(R)]
    out["xc"], out["yc"] = xc, yc
    sh = shifts_of(seed, m, P) if m >= 2 else []
    out["shift_values"] = sh
    for j in range(R):
        for f in range(F):
            T = table_of(xc[f], yc[j], M, H)
            out["tables"][j, f] = T
            dn, est, cu, hu = measures(T)
            out["delta_num"][j, f], out["classes_used"][j, f], out["cells_used"][j, f] = dn, cu, hu
            out["mi_cells"][j, f, 0] = np.count_nonzero(T)
            for k, key in enumerate(MEASURES):
                out[key]["estimate"][j, f] = est[k]
            for p, s in enumerate(sh):
                Tp = table_of(xc[f], np.roll(yc[j], -s), M, H)
                out["null_values"][j, f, :, p] = measures(Tp)[1]
                out["mi_cells"][j, f, 1 + p] = np.count_nonzero(Tp)
            if sh:
                for k, key in enumerate(MEASURES):
                    v = out["null_values"][j, f, k]
                    out[key]["null_mean"][j, f] = np.cumsum(v)[-1] / float(P)
                    out[key]["null_hi"][j, f] = np.quantile(v, level)
                    out[key]["exceed"][j, f] = int((v >= est[k]).sum())
            vs = variance_share(xc[f], fy[j], M)
            out["share"][j][f] = vs
            out["row_mean"][j], out["row_ss"][j] = float(vs["row_mean"]), float(vs["row_ss"])
            for key in ("eta2", "eta2_adj", "f_stat"):
                out[key][j, f] = float(vs[key])
            cs = out["class_stats"][j, f]
            cs[:, 0] = vs["count"]
            used = vs["count"] > 0
            cs[used, 1] = vs["mean"][used].astype(np.float64)
            cs[used, 2] = np.sqrt(vs["ss"][used] / vs["count"][used]).astype(np.float64)
            cs[:, 3:6] = class_x(fx[f], xc[f], M)
    return out


def ishigami_case(n=16384, seed=2024):
    """x [4, n] uniform on (-pi, pi) - the three inputs of the Ishigami function (a = 7, b = 0.1) and one dummy - and y [n]."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-np.pi, np.pi, (4, n))
    y = np.sin(x[0]) + 7.0 * np.sin(x[1]) ** 2 + 0.1 * x[2] ** 4 * np.sin(x[0])
    return x, y
