"""What test_reweight_abi.py (host) and test_gpu_reweight.py (device) share: the cases of erpl_mc_reweight and the comparison of
a result dict (analysis.reweight_result_dict plus 'logw' and 'weights') with another."""
import math

import numpy as np

import reweight_ref as R
from erpl_monte_carlo_sim_amd import _abi

N, U = _abi.DESIGN_NORMAL, _abi.DESIGN_UNIFORM
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 70001)
VARIANTS = ("one_row", "thirty_two_rows", "mixed", "extra_row", "constant_row")
REL = 1e-12          # the project's bar for erpl_mc_analyze against tests/golden/stats.json


def make_case(variant, n, seed=5, pad=0):
    """A case as the keyword arguments of analysis.reweight_host / TrajectoryEngine.reweight (NumPy).  pad > 0: `factors` and
    `summary` are views of wider matrices (ld = n + pad) whose other columns hold a sentinel no result may depend on."""
    rng = np.random.default_rng(seed + 1000 * VARIANTS.index(variant) + n)
    summary_full = np.full((_abi.SUMMARY_DIM, n + pad), 1e300)
    summary = summary_full[:, :n]
    summary[:] = rng.normal(size=(_abi.SUMMARY_DIM, n)) * 50.0 + 3000.0
    case = {"mask": None, "extra": None, "rows": None, "thresholds": None, "quantiles": (0.05, 0.25, 0.5, 0.75, 0.95)}
    if variant == "one_row":
        kinds, law = [N], [(0.4, 0.8)]
        case["thresholds"] = {_abi.SUM_RANGE: [3000.0, 3050.0]}
    elif variant == "thirty_two_rows":
        kinds = [N if r % 4 else U for r in range(32)]
        law = [(0.02 * (r % 5 - 2), 1.0 - 0.004 * r) if k == N else (0.01 * (r % 3), 1.0 - 0.005 * (r % 7)) for r, k in enumerate(kinds)]
        case["rows"] = [_abi.SUM_MAX_SPEED]
        case["quantiles"] = (0.0, 0.5, 1.0)
    elif variant == "mixed":
        kinds, law = [N, N, U, N], [(0.3, 0.7), (0.0, 0.5), (0.2, 0.6), (-0.2, 1.1)]
        case["rows"] = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, _abi.SUM_IMPACT_X]
        summary[_abi.SUM_RANGE] = np.round(summary[_abi.SUM_RANGE] / 25.0) * 25.0                    # ties
        summary[_abi.SUM_IMPACT_X] = np.where(rng.uniform(size=n) < 0.4, rng.choice([0.0, -0.0], size=n), rng.integers(-2, 3, n).astype(float))
        case["thresholds"] = {_abi.SUM_APOGEE_ALT: [2900.0, 3000.0, 3100.0, 1e9, -1e9], _abi.SUM_IMPACT_X: [-0.0, 0.0, 1.0]}
        case["quantiles"] = (0.0, 0.01, 0.3, 0.5, 0.7, 0.99, 1.0, 0.5)
        case["mask"] = (rng.uniform(size=n) < 0.1).astype(np.uint8)
    elif variant == "constant_row":          # one value in every column: a whole wave of non-zero weights adds into one bin
        kinds, law = [N], [(0.1, 0.9)]       # (the value is 0.0: its weighted mean is exact in every order of the sum, so the
        case["rows"] = [_abi.SUM_RANGE, _abi.SUM_APOGEE_ALT]   # centred moments are 0 and not the rounding of a mean)
        summary[_abi.SUM_RANGE] = 0.0
        case["thresholds"] = {_abi.SUM_RANGE: [0.0, -1.0]}
    else:
        kinds, law = [U, N], [(0.0, 0.75), (-0.5, 0.9)]
        case["rows"] = [_abi.RW_ROW_EXTRA, _abi.SUM_RANGE]
        case["extra"] = (rng.uniform(size=n) < 0.3).astype(np.float64)                               # a 0 / 1 zone indicator
        case["thresholds"] = {_abi.RW_ROW_EXTRA: [0.5]}
    factors_full = np.full((len(kinds), n + pad), -1e300)
    factors = factors_full[:, :n]
    for r, k in enumerate(kinds):
        factors[r] = rng.normal(size=n) if k == N else rng.uniform(size=n)
    if variant == "mixed" and n >= 63:       # NaN and +-inf in law rows and in outcome rows
        factors[0, 3], factors[1, 10], factors[2, 20], factors[3, 30] = math.nan, math.inf, math.nan, -math.inf
        summary[_abi.SUM_APOGEE_ALT, 5], summary[_abi.SUM_IMPACT_X, 11], summary[_abi.SUM_FLIGHT_TIME, n - 1] = math.nan, math.inf, -math.inf
        summary[_abi.SUM_MAX_SPEED, 40] = math.nan                                                    # not requested: no effect
    if variant == "extra_row" and n >= 63:
        case["extra"][7] = math.nan
    case.update(factors=factors, kinds=kinds, law=law, summary=summary)
    return case


def reference(case):
    rows = case["rows"] if case["rows"] is not None else (_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME)
    return R.reweight(case["factors"], case["kinds"], case["law"], case["summary"], mask=case["mask"], rows=tuple(rows), extra=case["extra"],
                      thresholds=case["thresholds"], quantiles=case["quantiles"])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def close(got, want, rel=REL, scale=None):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= rel * (abs(want) if scale is None else scale)


def mean_scales(case, weights):
    """sum W |x| / S of every requested row, from the weights of a result: the scale of the bar on the mean."""
    rows = case["rows"] if case["rows"] is not None else (_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME)
    w = np.asarray(weights).astype(np.float64)
    S = float(sum(int(v) for v in np.asarray(weights)))
    use = w > 0
    return {r: (math.fsum(w[use] * np.abs(R.outcome(case["summary"], case["extra"], r)[use])) / S if S else math.nan) for r in rows}


def compare(got, want, what="", scales=None):
    """Integers, logw, weights and quantiles byte for byte; every double within REL relative, the mean within
    REL * sum W |x| / S (the restatement's 'mean_scale', or `scales` = mean_scales(..) against a host result)."""
    for k in ("n", "count", "n_masked", "n_non_finite", "n_outside", "n_zero", "Q", "sum_w", "max_w"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    if "logw" in got and "logw" in want:
        assert np.array_equal(bits(got["logw"]), bits(want["logw"])), (what, "logw")
        assert np.array_equal(np.asarray(got["weights"]), np.asarray(want["weights"])), (what, "weights")
    for k in ("sum_w2", "ess", "ess_expected_share"):
        assert close(got[k], want[k]), (what, k, got[k], want[k])
    assert list(got["rows"]) == list(want["rows"]), (what, "rows")
    for r in got["rows"]:
        g, w = got["rows"][r], want["rows"][r]
        assert g["exceed_w"] == w["exceed_w"], (what, r, "exceed_w", g["exceed_w"], w["exceed_w"])
        assert np.array_equal(bits(g["quantiles"]), bits(w["quantiles"])), (what, r, "quantiles", g["quantiles"], w["quantiles"])
        for k in ("min", "max"):           # the value; which of two equal zeros an extreme keeps is the order's, not the contract's
            assert g[k] == w[k] or (math.isnan(g[k]) and math.isnan(w[k])), (what, r, k, g[k], w[k])
        scale = w["mean_scale"] if "mean_scale" in w else scales[r]
        assert close(g["mean"], w["mean"], scale=scale), (what, r, "mean", g["mean"], w["mean"])
        for k in ("mean_se", "var", "std"):
            assert close(g[k], w[k]), (what, r, k, g[k], w[k])
        for k in ("p", "p_se"):
            for a, b in zip(g[k], w[k]):
                assert close(a, b), (what, r, k, a, b)
