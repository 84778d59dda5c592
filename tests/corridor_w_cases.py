"""What test_corridor_w_ref.py (host) and test_gpu_corridor_w.py (device) share: the cases of erpl_mc_corridor_bands_weighted and
the comparison of a result dict (analysis.bands_weighted_result_dict) with another.  Small deterministic tables, C x T at most
2 x 5, ld > m with the padding poisoned (NaN and huge values; a result that read it shows).  m in {1, 63, 255, 257, 1025, 4099}:
either side of a wave, of a workgroup and of the four columns a thread keeps in flight."""
import math

import numpy as np

REL = 1e-12          # erpl_mc_reweight's bar between the device and the host twin
PAD = 5
EXACT = ("count", "n_non_finite", "n_zero", "sum_w", "exceed_w")
RECORD = ("m", "n_masked", "n_counted", "max_w", "K", "Q")
DOUBLES = ("var", "std", "mean_se", "sum_w2", "ess", "a2", "p", "p_se")


def q_bits(m):
    return min(52, 62 - (m - 1).bit_length())


def _matrix(rng, C, T, m, scale=50.0, centre=10.0):
    full = np.empty((C, T, m + PAD))
    full[:, :, :m] = rng.normal(size=(C, T, m)) * scale + centre
    full[:, :, m:] = np.array([math.nan, 1e300, -1e300, math.inf, 7e299])[:PAD]
    return full


def _case(values, m, weights, mask=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), thresholds=None):
    return {"values": values, "m": m, "weights": np.asarray(weights, dtype=np.int64), "mask": None if mask is None else
            np.asarray(mask, dtype=np.uint8), "quantiles": tuple(quantiles), "thresholds": thresholds}


def make_cases():
    """name -> case; a case is the arguments of analysis.bands_weighted_host / TrajectoryEngine.corridor_bands_weighted."""
    cases = {}
    # m = 1: one member; a row whose only value is NaN has an empty population
    v = _matrix(np.random.default_rng(1), 1, 2, 1)
    v[0, 0, 0], v[0, 1, 0] = 3.5, math.nan
    cases["m1"] = _case(v, 1, [5], quantiles=(0.0, 0.5, 1.0), thresholds=[[3.5, 3.0]])

    # m = 63: a row of one repeated value (a whole wave in one bin), zeros of both signs, NaN, both infinities, W = 0 columns,
    # a mask, thresholds equal to a value of the row; sum_w over the open columns a multiple of 4, so that 0.25 * sum_w is an
    # integer on the rows whose values are all finite
    rng = np.random.default_rng(63)
    m = 63
    v = _matrix(rng, 2, 3, m)
    v[0, 1, :m] = 2.0
    v[1, 0, :m:4] = np.tile([0.0, -0.0], m)[:len(v[1, 0, :m:4])]
    v[1, 0, 5], v[1, 0, 6], v[1, 0, 7] = math.nan, math.inf, -math.inf
    v[1, 2, :m] = np.round(v[1, 2, :m] / 25.0) * 25.0       # ties
    w = rng.integers(0, 10, m)
    mask = (rng.uniform(size=m) < 0.1).astype(np.uint8)
    mask[0] = 0
    w[0] = 1
    w[0] += (-int(w[mask == 0].sum())) % 4
    cases["m63"] = _case(v, m, w, mask, quantiles=(0.0, 0.25, 0.5, 1.0, 0.9), thresholds=[[2.0, 0.0], [-0.0, float(v[1, 2, 3]), 1e9, -1e9]])

    # m = 255: one column holds all but a few units of the weight
    rng = np.random.default_rng(255)
    m = 255
    # (integer values and weights below 2^21: w x and its sums are exact, so both sides divide the same two numbers for the mean.
    # With a rounded mean the heavy column's x - mean, of the size of that rounding, would carry mean_se - no bar on the sums holds
    # for that, by any order of addition)
    v = _matrix(rng, 1, 5, m)
    v[:, :, :m] = np.round(v[:, :, :m])
    w = np.zeros(m, dtype=np.int64)
    w[[3, 64, 128, 200, 254]] = 1
    w[100] = 1000000
    v[0, 2, 100] = math.nan                                  # the heavy column is no member of this row
    cases["m255"] = _case(v, m, w, thresholds=[[10.0]])

    # m = 257: ties, thresholds at values of the row, a second channel without thresholds
    rng = np.random.default_rng(257)
    m = 257
    v = _matrix(rng, 2, 2, m)
    v[:, :, :m] = np.round(v[:, :, :m])
    w = rng.integers(0, 1000, m)
    mask = (rng.uniform(size=m) < 0.2).astype(np.uint8)
    cases["m257"] = _case(v, m, w, mask, quantiles=(0.01, 0.5, 0.99), thresholds=[[float(v[0, 0, 0]), float(v[0, 1, 256])], []])

    # m = 1025: weights of every size up to 2^Q
    rng = np.random.default_rng(1025)
    m = 1025
    v = _matrix(rng, 1, 3, m)
    Q = q_bits(m)
    w = (rng.integers(0, 1 << 62, m) >> rng.integers(11, 63, m)).astype(np.int64)
    w[17], w[18], w[19] = 1 << Q, 0, 1
    v[0, 1, 1024], v[0, 1, 0] = math.nan, -math.inf
    cases["m1025"] = _case(v, m, w, quantiles=(0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 0.5), thresholds=[[10.0, 60.0, -40.0]])

    # m = 4099: every W = 2^Q, sum_w above 2^53; q * sum_w an integer at 0.25 (sum_w is a multiple of 2^49)
    rng = np.random.default_rng(4099)
    m = 4099
    v = _matrix(rng, 1, 2, m)
    v[0, 1, :m] = np.round(v[0, 1, :m] / 10.0) * 10.0
    cases["m4099"] = _case(v, m, np.full(m, 1 << q_bits(m)), quantiles=(0.0, 0.25, 0.5, 1.0), thresholds=[[10.0]])

    # all weights zero: every row empty, no refusal
    v = _matrix(np.random.default_rng(7), 1, 2, 63)
    v[0, 1, 3] = math.nan
    cases["all_zero"] = _case(v, 63, np.zeros(63, dtype=np.int64), thresholds=[[0.0]])

    # a mask that removes every column
    v = _matrix(np.random.default_rng(8), 2, 1, 257)
    cases["all_masked"] = _case(v, 257, np.random.default_rng(9).integers(0, 50, 257), np.ones(257, dtype=np.uint8))
    return cases


CASES = make_cases()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def mean_scales(case):
    """sum W |x| / S of every row over its own population, float64 [C, T] (NaN for an empty row): the scale of the bar on the mean."""
    v, m = case["values"], case["m"]
    C, T = v.shape[:2]
    out = np.full((C, T), math.nan)
    open_ = np.ones(m, dtype=bool) if case["mask"] is None else case["mask"] == 0
    for c in range(C):
        for k in range(T):
            x = v[c, k, :m]
            use = open_ & np.isfinite(x) & (case["weights"] > 0)
            S = sum(int(t) for t in case["weights"][use])
            if S:
                out[c, k] = math.fsum(case["weights"][use].astype(np.float64) * np.abs(x[use])) / float(S)
    return out


def close(got, want, scale=None):
    """Elementwise: NaN where NaN, otherwise within REL relative (of `scale`, if given)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    ref = np.abs(want) if scale is None else np.broadcast_to(scale, want.shape)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - want) <= REL * ref
    return bool(np.all(np.where(nan, np.isnan(got), ok)))


def compare(got, want, case, what=""):
    """The exact fields, the quantiles and the extremes byte for byte; every double within REL relative, the mean within
    REL * sum W |x| / S."""
    for k in RECORD:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in EXACT:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("quantiles", "min", "max"):
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (what, k, got[k], want[k])
    assert close(got["mean"], want["mean"], mean_scales(case)), (what, "mean", got["mean"], want["mean"])
    for k in DOUBLES:
        assert got[k].shape == want[k].shape and close(got[k], want[k]), (what, k, got[k], want[k])
    assert got["q"] == want["q"] and got["thresholds"] == want["thresholds"], (what, "spec")


def same_bytes(a, b):
    """Two results of one call: everything, the doubles included, bit for bit."""
    for k in a:
        if isinstance(a[k], np.ndarray):
            same = a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        else:
            same = a[k] == b[k]
        if not same:
            return False
    return set(a) == set(b)
