"""A NumPy restatement of erpl_mc_reweight (csrc/erpl_reweight.h), one operation at a time: the yardstick of
test_reweight_abi.py.  The log-weights and the portable exp are float64 ufuncs (each rounds once, no FMA); c_r comes from
math.log, the libm of the library's host code; W, S, the exceedances and the ranks are Python ints / uint64; the quantiles
come from a stable sort on the library's key and a cumulative sum of W.  The sums of doubles are math.fsum of the rounded
terms: the exact sum, rounded once - no order of addition to argue about."""
import math

import numpy as np

NORMAL, UNIFORM = 1, 0                       # _abi.DESIGN_NORMAL, _abi.DESIGN_UNIFORM
ROW_EXTRA = 16
LOG2E = 1.4426950408889634
LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
COEF = (1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889,
        0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08,
        2.08767569878681e-09, 1.6059043836821613e-10)          # 1 / j!, j = 0 .. 13


def rw_exp(x):
    """erpl_rw_exp of every element: 0 below -64 and for a NaN."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(x.shape)
    with np.errstate(invalid="ignore"):
        use = x >= -64.0
    v = x[use]
    k = np.rint(v * LOG2E)
    hi, lo = k * LN2_HI, k * LN2_LO
    r = (v - hi) - lo
    s = np.full(v.shape, COEF[13])
    for c in COEF[12::-1]:
        s = s * r
        s = s + c
    out[use] = np.ldexp(s, k.astype(np.int64))
    return out


def q_bits(n):
    return min(52, 62 - (n - 1).bit_length())                  # ceil(log2 n) = bit_length(n - 1)


def key_of(x):
    """The library's order-preserving key (erpl_tally_key): -0.0 just below +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def outcome(summary, extra, row):
    return extra if row == ROW_EXTRA else summary[row]


def log_weights(factors, kinds, law, summary, extra, mask, rows):
    """(l float64 [n]: NaN where masked or non-finite, -inf outside the support; state int [n]: 0 in, 1 masked, 2 non-finite,
    3 outside)."""
    n = factors.shape[1]
    l = np.zeros(n)
    finite = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for r, (kind, p) in enumerate(zip(kinds, law)):
            x = factors[r]
            finite &= np.isfinite(x)
            if kind == NORMAL:
                mu, s = p
                c = -math.log(s)
                t = (x - mu) / s
                zz, tt = x * x, t * t
                d = zz - tt
                lr = c + 0.5 * d
            else:
                a, b = p
                c = -math.log(b - a)
                lr = np.where((a <= x) & (x <= b), c, -np.inf)
            l = l + lr
        for row in rows:
            finite &= np.isfinite(outcome(summary, extra, row))
        masked = np.zeros(n, dtype=bool) if mask is None else np.asarray(mask) != 0
        state = np.zeros(n, dtype=np.int64)
        outside = ~(l > -np.inf)
    state[outside] = 3
    state[~finite] = 2
    state[masked] = 1
    out = np.where(state == 0, l, np.where(state == 3, -np.inf, np.nan))
    return out, state


def reweight(factors, kinds, law, summary, mask=None, rows=(0, 4, 5), extra=None, thresholds=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95)):
    """The dict of analysis.reweight_result_dict plus 'logw', 'weights' and per row 'mean_scale' = sum W |x| / S."""
    factors = np.asarray(factors, dtype=np.float64)
    n = factors.shape[1]
    thresholds = thresholds or {}
    l, state = log_weights(factors, kinds, law, summary, extra, mask, rows)
    Q = q_bits(n)
    pop = state == 0
    W = np.zeros(n, dtype=np.int64)
    count = int(pop.sum())
    if count:
        lmax = l[pop].max()
        with np.errstate(invalid="ignore"):
            W[pop] = np.floor(np.ldexp(rw_exp(l[pop] - lmax), Q)).astype(np.int64)
    S = sum(int(v) for v in W)
    out = {"n": n, "count": count, "n_masked": int((state == 1).sum()), "n_non_finite": int((state == 2).sum()),
           "n_outside": int((state == 3).sum()), "n_zero": int((pop & (W == 0)).sum()), "Q": Q, "logw": l, "weights": W, "rows": {}}
    empty = count == 0 or S == 0
    wd = W.astype(np.float64)
    sum_w2 = math.fsum(wd * wd)
    Sd = float(S)
    out["sum_w"], out["max_w"] = (0, 0) if empty else (S, int(W.max()))
    out["sum_w2"], out["ess"] = (math.nan, math.nan) if empty else (sum_w2, Sd * Sd / sum_w2)
    out["ess_expected_share"] = expected_share(kinds, law)
    use = W > 0
    for row in rows:
        thr = [float(t) for t in thresholds.get(row, ())]
        qs = [float(q) for q in quantiles]
        rec = {"q": qs, "thresholds": thr}
        if empty:
            rec.update(mean=math.nan, mean_se=math.nan, var=math.nan, std=math.nan, min=math.nan, max=math.nan, mean_scale=math.nan,
                       quantiles=[math.nan] * len(qs), exceed_w=[0] * len(thr), p=[math.nan] * len(thr), p_se=[math.nan] * len(thr))
            out["rows"][row] = rec
            continue
        x = np.where(use, outcome(summary, extra, row), 0.0)
        w = wd[use]
        xv = x[use]
        mean = math.fsum(w * xv) / Sd
        d = xv - mean
        dd = d * d
        m2, se2 = math.fsum(w * dd), math.fsum((w * w) * dd)
        var = m2 / Sd
        rec.update(mean=mean, mean_se=math.sqrt(se2) / Sd, var=var, std=math.sqrt(var), min=float(xv.min()), max=float(xv.max()),
                   mean_scale=math.fsum(w * np.abs(xv)) / Sd)
        order = np.argsort(key_of(xv), kind="stable")
        cum = np.cumsum(W[use][order].astype(np.uint64))
        rec["quantiles"] = []
        for q in qs:
            T = min(max(int(math.ceil(q * Sd)), 1), S)
            rec["quantiles"].append(float(xv[order][int(np.searchsorted(cum, np.uint64(T), side="left"))]))
        rec["exceed_w"], rec["p"], rec["p_se"] = [], [], []
        for t in thr:
            over = xv > t
            e = sum(int(v) for v in W[use][over])
            a2 = math.fsum((w * w)[over])
            p = float(e) / Sd
            v = (1.0 - 2.0 * p) * a2 + (p * p) * sum_w2
            rec["exceed_w"].append(e)
            rec["p"].append(p)
            rec["p_se"].append(math.sqrt(max(v, 0.0)) / Sd)
        out["rows"][row] = rec
    return out


def expected_share(kinds, law):
    """1 / prod_r E[w_r^2]; 0 where a normal row has s^2 >= 2."""
    prod = 1.0
    for kind, p in zip(kinds, law):
        if kind == NORMAL:
            mu, s = p
            v = 2.0 - s * s
            if not v > 0.0:
                return 0.0
            prod *= math.exp(mu * mu / v) / (s * math.sqrt(v))
        else:
            prod *= 1.0 / (p[1] - p[0])
    return 1.0 / prod
