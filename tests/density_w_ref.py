"""The rule of erpl_mc_impact_density_weighted (include/erpl_mc.h) restated in NumPy: the population under integer weights,
the scaled weights, the weighted moments and the `neff` bandwidth of scipy.stats.gaussian_kde(weights=), the density through
the Cholesky-whitened coordinates, the exact zone weights and the weighted thresholds of the regions.  No device, no library:
tests/test_density_w_ref.py checks it against scipy and NumPy, tests/test_gpu_density_w.py checks the device against it."""
import math

import numpy as np


def rw_q(n):
    """Q of erpl_mc_reweight: min(52, 62 - ceil(log2 n)); a weight is admitted in 0 .. 2^Q."""
    return min(52, 62 - max(0, (int(n) - 1).bit_length()))


def population(x, y, W, mask=None):
    """(counted [n] bool, n_masked, n_non_finite, n_zero): the samples in the order the header counts them."""
    x, y, W = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(W, dtype=np.int64)
    masked = np.zeros(len(x), dtype=bool) if mask is None else np.asarray(mask) != 0
    bad = ~masked & ~(np.isfinite(x) & np.isfinite(y))
    zero = ~masked & ~bad & (W == 0)
    return ~masked & ~bad & ~zero, int(masked.sum()), int(bad.sum()), int(zero.sum())


def scaled(W):
    """(w, S_d, K, sum_w, max_w) of the counted weights W (all > 0): w = W 2^-K with K the bit length of max_w - exact."""
    W = np.asarray(W, dtype=np.int64)
    sum_w, max_w = int(W.astype(object).sum()) if len(W) else 0, int(W.max()) if len(W) else 0
    K = max_w.bit_length()
    return np.ldexp(W.astype(np.float64), -K), math.ldexp(float(sum_w), -K), K, sum_w, max_w


def moments(x, y, W):
    """mean [2], cov [2, 2] (np.cov(aweights=W, bias=False)), sum_w2 (scaled), ess - of the counted points."""
    w, s_d, _, _, _ = scaled(W)
    mean = np.array([(w * x).sum() / s_d, (w * y).sum() / s_d])
    sum_w2 = float((w * w).sum())
    dx, dy = x - mean[0], y - mean[1]
    dof = s_d - sum_w2 / s_d
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = np.array([[(w * (dx * dx)).sum(), (w * (dx * dy)).sum()], [(w * (dx * dy)).sum(), (w * (dy * dy)).sum()]]) / dof
    return mean, cov, sum_w2, s_d * s_d / sum_w2


def bandwidth(cov, ess, bw_scale=1.0):
    """ERPL_BW_SCOTT: H = (bw_scale ess^(-1/6))^2 cov - scipy's scotts_factor on neff, d = 2."""
    f = bw_scale * ess ** (-1.0 / 6.0)
    return (f * f) * np.asarray(cov, dtype=np.float64)


def _whiten(Hm, mean):
    hxx, hxy, hyy = Hm[0][0], Hm[0][1], Hm[1][1]
    c11 = math.sqrt(hxx)
    c21 = hxy / c11
    c22 = math.sqrt(hyy - c21 * c21)
    w11, w22 = 1.0 / c11, 1.0 / c22
    w21 = -c21 * w11 * w22

    def to(px, py):
        dx, dy = np.asarray(px, dtype=np.float64) - mean[0], np.asarray(py, dtype=np.float64) - mean[1]
        return w11 * dx, w21 * dx + w22 * dy
    return to


def density(qx, qy, px, py, W, Hm, mean=None):
    """f(q) = norm sum_i w_i exp(-(q - p_i)' H^-1 (q - p_i) / 2), norm = 1 / (S_d 2 pi sqrt(det)), through the whitened
    coordinates of the header (centred on `mean`, default the weighted mean)."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    w, s_d, _, _, _ = scaled(W)
    if mean is None:
        mean = [(w * px).sum() / s_d, (w * py).sum() / s_d]
    to = _whiten(Hm, mean)
    (pu, pv), (qu, qv) = to(px, py), to(qx, qy)
    det = Hm[0][0] * Hm[1][1] - Hm[0][1] * Hm[0][1]
    out = np.zeros(len(qu))
    step = max(1, 2_000_000 // max(len(qu), 1))
    for s in range(0, len(pu), step):
        du, dv = qu[:, None] - pu[None, s:s + step], qv[:, None] - pv[None, s:s + step]
        out += (w[None, s:s + step] * np.exp(-0.5 * (du * du + dv * dv))).sum(axis=1)
    return out / (s_d * (2.0 * math.pi) * math.sqrt(det))


def density_unweighted(qx, qy, px, py, Hm, mean=None):
    """The unweighted map (erpl_mc_impact_density) restated the same way: every point once, norm = 1 / (m 2 pi sqrt(det))."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    if mean is None:
        mean = [px.mean(), py.mean()]
    to = _whiten(Hm, mean)
    (pu, pv), (qu, qv) = to(px, py), to(qx, qy)
    det = Hm[0][0] * Hm[1][1] - Hm[0][1] * Hm[0][1]
    out = np.zeros(len(qu))
    step = max(1, 2_000_000 // max(len(qu), 1))
    for s in range(0, len(pu), step):
        du, dv = qu[:, None] - pu[None, s:s + step], qv[:, None] - pv[None, s:s + step]
        out += np.exp(-0.5 * (du * du + dv * dv)).sum(axis=1)
    return out / (len(pu) * (2.0 * math.pi) * math.sqrt(det))


def crossing(vx, vy, x, y):
    """The even-odd rule of include/erpl_mc.h, every operation rounded on its own."""
    inside = np.zeros(len(x), dtype=bool)
    nv = len(vx)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(nv):
            j = i - 1 if i else nv - 1
            straddles = (vy[i] > y) != (vy[j] > y)
            left = x < (vx[j] - vx[i]) * (y - vy[i]) / (vy[j] - vy[i]) + vx[i]
            inside ^= straddles & left
    return inside


def zone_weight(poly, x, y, W):
    """sum W [inside], a Python int."""
    poly = np.asarray(poly, dtype=np.float64)
    inside = crossing(poly[:, 0], poly[:, 1], np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    return int(np.asarray(W, dtype=np.int64)[inside].astype(object).sum()) if inside.any() else 0


def target_rank(level, sum_w):
    """T = clamp(ceil((1 - level) * (double) sum_w), 1, sum_w)."""
    return min(max(int(math.ceil((1.0 - level) * float(sum_w))), 1), sum_w)


def thresholds(f, W, levels):
    """t_k: the value at 0-based rank T_k - 1 of the multiset in which f_j occurs W_j times (integer arithmetic)."""
    f, W = np.asarray(f, dtype=np.float64), np.asarray(W, dtype=np.int64)
    order = np.argsort(f, kind="stable")
    cum = np.cumsum(W[order].astype(object))
    sum_w = int(cum[-1])
    out = []
    for p in levels:
        T = target_rank(p, sum_w)
        lo, hi = 0, len(cum) - 1
        while lo < hi:   # the first position whose cumulative weight reaches T
            mid = (lo + hi) // 2
            if cum[mid] >= T:
                hi = mid
            else:
                lo = mid + 1
        out.append(float(f[order[lo]]))
    return out


def content_w(f, W, t):
    """sum W [f >= t], a Python int."""
    sel = np.asarray(f, dtype=np.float64) >= t
    return int(np.asarray(W, dtype=np.int64)[sel].astype(object).sum()) if sel.any() else 0
