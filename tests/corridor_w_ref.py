"""A NumPy restatement of erpl_mc_corridor_bands_weighted (csrc/erpl_bands_w.h), one operation at a time: the yardstick of
test_corridor_w_ref.py.  W, sum_w, the exceedances and the ranks are Python ints; the quantiles come from a stable sort on the
library's key and a cumulative sum of W; the scaled weights are np.ldexp (exact); the sums of doubles are math.fsum of the
rounded terms: the exact sum, rounded once - no order of addition to argue about."""
import math

import numpy as np

MAX_THRESHOLDS = 4


def q_bits(m):
    return min(52, 62 - (m - 1).bit_length())                  # ceil(log2 m) = bit_length(m - 1)


def key_of(x):
    """The library's order-preserving key (erpl_tally_key): -0.0 just below +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def first_bad(weights, m):
    """The lowest column whose weight is outside 0 .. 2^Q, or -1."""
    most = 1 << q_bits(m)
    for i in range(m):
        if not 0 <= int(weights[i]) <= most:
            return i
    return -1


def bands_weighted(values, weights, mask=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), thresholds=None, m=None):
    """The dict of analysis.bands_weighted_result_dict."""
    values = np.asarray(values, dtype=np.float64)
    C, T, ld = values.shape
    m = ld if m is None else m
    W = [int(v) for v in np.asarray(weights)[:m]]
    assert first_bad(W, m) < 0
    open_ = np.ones(m, dtype=bool) if mask is None else np.asarray(mask)[:m] == 0
    max_w = max(W)
    K = max_w.bit_length()
    qs = [float(q) for q in quantiles]
    thr = [[] for _ in range(C)]
    if thresholds is not None:
        for c, t in (thresholds.items() if hasattr(thresholds, "items") else enumerate(thresholds)):
            thr[c] = [float(x) for x in (t or ())]
    out = {k: np.zeros((C, T), dtype=np.int64) for k in ("count", "n_non_finite", "n_zero", "sum_w")}
    out.update({k: np.full((C, T), math.nan) for k in ("min", "max", "mean", "var", "std", "mean_se", "sum_w2", "ess")})
    out["quantiles"] = np.full((C, len(qs), T), math.nan)
    out["exceed_w"] = np.zeros((C, MAX_THRESHOLDS, T), dtype=np.int64)
    for k in ("a2", "p", "p_se"):
        out[k] = np.full((C, MAX_THRESHOLDS, T), math.nan)
    Wa = np.array(W, dtype=np.int64)
    for c in range(C):
        for k in range(T):
            x = values[c, k, :m]
            finite = np.isfinite(x)
            member = open_ & finite & (Wa > 0)
            out["n_non_finite"][c, k] = int((open_ & ~finite).sum())
            out["n_zero"][c, k] = int((open_ & finite & (Wa == 0)).sum())
            S = sum(W[i] for i in np.flatnonzero(member))
            if S == 0:
                continue
            xv, Wv = x[member], Wa[member]
            w = np.ldexp(Wv.astype(np.float64), -K)
            Sd = math.ldexp(float(S), -K)
            out["count"][c, k], out["sum_w"][c, k] = int(member.sum()), S
            mean = math.fsum(w * xv) / Sd
            d = xv - mean
            dd = d * d
            var = math.fsum(w * dd) / Sd
            sum_w2 = math.fsum(w * w)
            out["mean"][c, k], out["var"][c, k], out["std"][c, k] = mean, var, math.sqrt(var)
            out["mean_se"][c, k] = math.sqrt(math.fsum((w * w) * dd)) / Sd
            out["sum_w2"][c, k], out["ess"][c, k] = sum_w2, Sd * Sd / sum_w2
            order = np.argsort(key_of(xv), kind="stable")
            xs = xv[order]
            out["min"][c, k], out["max"][c, k] = xs[0], xs[-1]
            cum, run = [], 0
            for v in Wv[order]:
                run += int(v)
                cum.append(run)
            for j, q in enumerate(qs):
                t = math.ceil(q * float(S))
                t = min(max(int(t), 1), S)
                lo, hi = 0, len(cum) - 1       # the first position whose cumulative weight reaches t
                while lo < hi:
                    mid = (lo + hi) // 2
                    if cum[mid] >= t:
                        hi = mid
                    else:
                        lo = mid + 1
                out["quantiles"][c, j, k] = xs[lo]
            for j, t in enumerate(thr[c]):
                over = xv > t
                e = sum(int(v) for v in Wv[over])
                a2 = math.fsum((w * w)[over])
                p = float(e) / float(S)
                v = (1.0 - 2.0 * p) * a2 + (p * p) * sum_w2
                out["exceed_w"][c, j, k], out["a2"][c, j, k] = e, a2
                out["p"][c, j, k], out["p_se"][c, j, k] = p, math.sqrt(max(v, 0.0)) / Sd
    out["q"], out["thresholds"] = qs, thr
    out.update(m=m, n_masked=int((~open_).sum()), n_counted=int(open_.sum()), max_w=max_w, K=K, Q=q_bits(m))
    return out
