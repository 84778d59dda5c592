"""erpl_mc_correlation on the device against NumPy / SciPy on host copies of the same tensors.

Exact, no tolerance: count, n_masked, n_non_finite, constant, min, max, and every mid-rank (scipy.stats.rankdata, method
'average', of the population; NaN elsewhere).
Rounded: corr, rank_corr, pearson, spearman against the centred-Gram formula in np.longdouble, absolute error <= 1e-12
(the bar of test_gpu_analysis.py; on the CPU float64 two-pass, np.corrcoef and scipy.stats.spearmanr sit within 7e-16
of long double at n = 100 003, V = 35, so the bar leaves three decades for another summation order); mean at
1e-12 * mean|x| and std at 1e-12 * std as that file scales them; src / srrc / r2 / r2_rank against np.linalg.solve on the
long-double matrix rounded to float64, at 1e-12 * cond(R_ff)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy.stats import rankdata

from erpl_monte_carlo_sim_amd import _abi, analysis, models, plots

import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-12
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 4097, 100003)


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


# ------------------------------------------------------------------ host reference
def gram_corr(P, constant):
    """corr of the rows of P ([V, count]) by the centred-Gram formula in long double; NaN where a variable is constant."""
    L = P.astype(np.longdouble)
    d = L - L.mean(axis=1, keepdims=True)
    S = d @ d.T
    with np.errstate(invalid="ignore", divide="ignore"):
        c = S / np.sqrt(np.outer(np.diag(S), np.diag(S)))
    c[constant, :] = np.nan
    c[:, constant] = np.nan
    return c


def regression(corr, F, R, constant):
    """(coefficients [R, F], r2 [R], cond(R_ff), separable) by np.linalg.solve on the float64 rounding of `corr`; separable:
    every Cholesky pivot of R_ff (1 - R^2 of a factor on the ones before it) is at least 1e-10."""
    c = np.asarray(corr, dtype=np.float64)
    use = [f for f in range(F) if not constant[f]]
    beta, r2 = np.full((R, F), np.nan), np.full(R, np.nan)
    cond = 1.0
    if use:
        rff = c[np.ix_(use, use)]
        cond = np.linalg.cond(rff)
        L = np.zeros_like(rff)
        for i in range(len(use)):
            for k in range(i + 1):
                t = rff[i, k] - L[i, :k] @ L[k, :k]
                if i == k:
                    if not t >= 1e-10:
                        return beta, r2, cond, False
                    L[i, i] = np.sqrt(t)
                else:
                    L[i, k] = t / L[k, k]
        for j in range(R):
            if not constant[F + j]:
                b = np.linalg.solve(rff, c[F + j, use])
                beta[j, use] = b
                r2[j] = float(b @ c[F + j, use])
    else:
        r2[[j for j in range(R) if not constant[F + j]]] = 0.0
    return beta, r2, cond, True


def reference(fac, summ, mask, rows):
    X = np.vstack([fac, summ[rows]])
    V, n = X.shape
    m = np.zeros(n, dtype=bool) if mask is None else mask != 0
    fin = np.isfinite(X).all(axis=0)
    pop = ~m & fin
    ref = {"count": int(pop.sum()), "n_masked": int(m.sum()), "n_non_finite": int((~m & ~fin).sum()), "pop": pop}
    P = X[:, pop]
    ref["P"] = P
    if P.shape[1] == 0:
        return ref
    ref["min"], ref["max"] = P.min(axis=1), P.max(axis=1)
    ref["constant"] = ref["min"] == ref["max"]
    ref["mean"], ref["std"] = P.mean(axis=1), P.std(axis=1)
    ref["corr"] = gram_corr(P, ref["constant"])
    rk = np.vstack([rankdata(P[v], method="average") for v in range(V)])
    ref["ranks"] = np.full((V, n), np.nan)
    ref["ranks"][:, pop] = rk
    ref["rank_corr"] = gram_corr(rk, ref["constant"])
    return ref


def close(got, want, tol=TOL):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    err = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
    assert err <= tol, (err, tol)
    return err


def dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def check(engine, fac, summ, mask, rows, ranks=True, expect_ok=None, label=""):
    """One call against the host reference; returns (device dict, reference)."""
    F, R = fac.shape[0], len(rows)
    V = F + R
    out = engine.correlation(dev(engine, fac), dev(engine, summ), None if mask is None else dev(engine, mask), rows=rows,
                             ranks=ranks, want_ranks=ranks)
    ref = reference(fac, summ, mask, rows)
    assert out["n"] == fac.shape[1]
    assert (out["count"], out["n_masked"], out["n_non_finite"]) == (ref["count"], ref["n_masked"], ref["n_non_finite"])
    assert out["count"] + out["n_masked"] + out["n_non_finite"] == fac.shape[1]
    if ranks:
        got_ranks = out["ranks"].cpu().numpy()
        assert got_ranks.shape == (V, fac.shape[1])
    if ref["count"] == 0:
        for k in ("mean", "std", "min", "max", "pearson", "spearman", "src", "srrc", "r2", "r2_rank", "corr"):
            assert np.isnan(out[k]).all(), k
        assert not out["regression_ok"] and not out["rank_regression_ok"]
        if ranks:
            assert np.isnan(out["rank_corr"]).all() and np.isnan(got_ranks).all()
        return out, ref
    assert np.array_equal(out["constant"] != 0, ref["constant"])
    assert np.array_equal(out["min"], ref["min"]) and np.array_equal(out["max"], ref["max"])
    scale = np.mean(np.abs(ref["P"]), axis=1)
    e_mean = np.max(np.abs(out["mean"] - ref["mean"]) / np.where(scale > 0, scale, 1.0))
    nz = ~ref["constant"]
    e_std = np.max(np.abs(out["std"] - ref["std"])[nz] / ref["std"][nz]) if nz.any() else 0.0
    assert e_mean <= TOL and e_std <= TOL, (e_mean, e_std)
    assert np.all(out["std"][~nz] <= TOL * np.abs(ref["min"][~nz]))       # a constant column: rounding of sum / count at most
    e_corr = close(out["corr"], ref["corr"])
    close(out["pearson"], ref["corr"][F:, :F])
    assert np.array_equal(out["pearson"], out["corr"][F:, :F], equal_nan=True)
    assert np.array_equal(out["corr"], out["corr"].T, equal_nan=True)
    assert np.all(np.diag(out["corr"])[~ref["constant"]] == 1.0)
    beta, r2, cond, ok = regression(ref["corr"], F, R, ref["constant"])
    assert expect_ok is None or ok == expect_ok
    e_rank = 0.0
    if ok:
        assert out["regression_ok"]
        close(out["src"], beta, TOL * cond)
        close(out["r2"], r2, TOL * cond)
    else:
        assert not out["regression_ok"] and np.isnan(out["src"]).all() and np.isnan(out["r2"]).all()
    if ranks:
        assert got_ranks.tobytes() == ref["ranks"].tobytes()          # bitwise: exact multiples of 0.5, NaN outside
        e_rank = close(out["rank_corr"], ref["rank_corr"])
        close(out["spearman"], ref["rank_corr"][F:, :F])
        assert np.array_equal(out["spearman"], out["rank_corr"][F:, :F], equal_nan=True)
        beta_r, r2_r, cond_r, ok_r = regression(ref["rank_corr"], F, R, ref["constant"])
        assert expect_ok is None or ok_r == expect_ok
        if ok_r:
            assert out["rank_regression_ok"]
            close(out["srrc"], beta_r, TOL * cond_r)
            close(out["r2_rank"], r2_r, TOL * cond_r)
            cond = max(cond, cond_r)
        else:
            assert not out["rank_regression_ok"] and np.isnan(out["srrc"]).all() and np.isnan(out["r2_rank"]).all()
    else:
        assert out["rank_corr"] is None and not out["rank_regression_ok"]
        for k in ("spearman", "srrc", "r2_rank"):
            assert np.isnan(out[k]).all(), k
    print(f"{label} n {fac.shape[1]} F {F} R {R} count {ref['count']}: mean err {e_mean:.1e}, std err {e_std:.1e}, "
          f"corr err {e_corr:.1e}, rank corr err {e_rank:.1e}, cond(R_ff) {cond:.3g}")
    return out, ref


def synthetic(n, F, rows, seed, dirty=True):
    """Factors like 1 + 0.02 z, uniform and heavily tied columns; outcomes that depend on them; a -0.0 / +0.0 pair, +-inf and
    NaN sprinkled into factors and rows."""
    rng = np.random.RandomState(seed)
    fac = np.empty((F, n))
    for f in range(F):
        kind = f % 3
        if kind == 0:
            fac[f] = 1.0 + 0.02 * rng.normal(size=n)
        elif kind == 1:
            fac[f] = rng.uniform(0.0, 5.0, n)
        else:
            fac[f] = np.round(rng.normal(size=n), 1)          # heavy ties; holds -0.0 and +0.0
    summ = rng.normal(size=(16, n)) * 3.0
    w = rng.normal(size=(len(rows), F))
    for j, r in enumerate(rows):
        summ[r] = 100.0 * (j + 1) + w[j] @ (fac - fac.mean(axis=1, keepdims=True)) + 0.3 * rng.normal(size=n)
        if j % 2:
            summ[r] = np.round(summ[r], 1)
    if n >= 2:
        fac[F - 1, 0], fac[F - 1, 1] = -0.0, 0.0
    if dirty and n >= 63:
        for k in range(max(2, n // 50)):
            v, i = rng.randint(F + len(rows)), rng.randint(2, n)
            val = (np.nan, np.inf, -np.inf)[k % 3]
            if v < F:
                fac[v, i] = val
            else:
                summ[rows[v - F], i] = val
        summ[[r for r in range(16) if r not in rows][:1], 5] = np.nan       # a row that was not asked for does not count
    return fac, summ


def shape_of(n):
    """(F, rows in non-sorted order) used at size n: every shape of the issue appears at some size."""
    if n == 100003:
        return 19, [_abi.SUM_RANGE, _abi.SUM_APOGEE_ALT, _abi.SUM_FLIGHT_TIME]
    if n == 4097:
        return 32, [15, 3, 7, 0, 9, 1, 14, 2, 13, 4, 12, 5, 11, 6, 10, 8]
    if n in (3, 65, 257):
        return 1, [_abi.SUM_FLIGHT_TIME]
    return 2, [_abi.SUM_RAIL_EXIT_SPEED, _abi.SUM_APOGEE_ALT, _abi.SUM_RANGE]


@pytest.mark.parametrize("n", SIZES)
def test_correlation_and_ranks_against_numpy_and_scipy(engine, n):
    F, rows = shape_of(n)
    fac, summ = synthetic(n, F, rows, seed=n)
    rng = np.random.RandomState(n + 1)
    random_mask = (rng.uniform(size=n) < 0.2).astype(np.uint8) * rng.randint(1, 64, n).astype(np.uint8)
    for label, mask in (("NULL", None), ("zero", np.zeros(n, dtype=np.uint8)), ("random", random_mask),
                        ("all", np.full(n, 3, dtype=np.uint8))):
        _, ref = check(engine, fac, summ, mask, rows, label=f"mask {label}")
        if label == "all":
            assert ref["count"] == 0
    if n >= 63:
        check(engine, fac, summ, random_mask, rows, ranks=False, label="no ranks")


def test_small_populations(engine):
    fac, summ = synthetic(64, 2, [0, 4, 5], seed=9, dirty=False)
    one = np.ones(64, dtype=np.uint8)
    one[17] = 0
    out, ref = check(engine, fac, summ, one, [0, 4, 5], label="count 1")
    assert out["count"] == 1 and np.all(out["constant"] == 1) and np.isnan(out["corr"]).all()
    assert out["ranks"][:, 17].tolist() == [1.0] * 5
    out, ref = check(engine, fac, summ, np.ones(64, dtype=np.uint8), [0, 4, 5], label="count 0")
    assert out["count"] == 0 and out["n_masked"] == 64


def test_constant_factor_is_dropped_and_changes_nothing_else(engine):
    n, rows = 5000, [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE]
    fac, summ = synthetic(n, 4, rows, seed=21)
    base, _ = check(engine, fac, summ, None, rows, label="without the constant factor")
    fac5 = np.vstack([fac[:2], np.full((1, n), 0.1), fac[2:]])      # 0.1 does not survive sum / count exactly
    out, ref = check(engine, fac5, summ, None, rows, label="with it")
    assert out["constant"].tolist() == [0, 0, 1, 0, 0, 0, 0]
    assert np.isnan(out["pearson"][:, 2]).all() and np.isnan(out["spearman"][:, 2]).all()
    assert np.isnan(out["src"][:, 2]).all() and np.isnan(out["srrc"][:, 2]).all()
    keep = [0, 1, 3, 4]
    for k in ("pearson", "spearman", "src", "srrc"):
        assert np.array_equal(out[k][:, keep], base[k]), k          # the same bits as the run without it
    assert np.array_equal(out["r2"], base["r2"]) and np.array_equal(out["r2_rank"], base["r2_rank"])


def test_duplicated_factor_is_reported_not_hidden(engine):
    n, rows = 3000, [_abi.SUM_RANGE, _abi.SUM_APOGEE_ALT]
    fac, summ = synthetic(n, 3, rows, seed=22)
    fac4 = np.vstack([fac, 3.0 * fac[0:1] - 7.0])                   # an exact affine image of factor 0
    out, _ = check(engine, fac4, summ, None, rows, expect_ok=False, label="duplicated factor")
    assert not np.isnan(out["pearson"]).any() and not np.isnan(out["spearman"]).any()


def test_constant_output_row(engine):
    n, rows = 1000, [_abi.SUM_APOGEE_ALT, _abi.SUM_FLIGHT_TIME, _abi.SUM_RANGE]
    fac, summ = synthetic(n, 3, rows, seed=23)
    summ[_abi.SUM_FLIGHT_TIME] = 600.0
    out, _ = check(engine, fac, summ, None, rows, label="constant row")
    assert out["constant"].tolist() == [0, 0, 0, 0, 1, 0]
    assert np.isnan(out["pearson"][1]).all() and np.isnan(out["src"][1]).all() and np.isnan(out["r2"][1])
    assert not np.isnan(out["src"][[0, 2]]).any()


def test_monotone_output_has_the_ranks_of_its_input(engine):
    n = 4097
    rng = np.random.RandomState(24)
    fac = np.vstack([np.round(rng.normal(size=n), 2), rng.normal(size=n)])
    summ = rng.normal(size=(16, n))
    summ[_abi.SUM_MAX_SPEED] = np.exp(fac[0])
    out, _ = check(engine, fac, summ, None, [_abi.SUM_MAX_SPEED], label="exp(x)")
    rk = out["ranks"].cpu().numpy()
    assert np.array_equal(rk[2], rk[0])
    assert abs(out["spearman"][0, 0] - 1.0) <= TOL and out["pearson"][0, 0] < 0.999


# ------------------------------------------------------------------ the C call itself
def raw_call(engine, fac, summ, mask, rows, stream=None):
    """erpl_mc_correlation through ctypes: (bytes of the result struct, corr, rank_corr, ranks tensor)."""
    F, n = fac.shape
    V = F + len(rows)
    spec = _abi.ErplCorrSpec()
    assert engine.lib.erpl_mc_correlation_defaults(C.byref(spec)) == 0
    spec.n_factors, spec.n_rows = F, len(rows)
    spec.rows[:len(rows)] = rows
    res = _abi.ErplCorrResult()
    corr, rank_corr = np.full((V, V), 7.0), np.full((V, V), 7.0)
    ranks = torch.full((V, n), 7.0, dtype=torch.float64, device=engine.device)
    st = stream if stream is not None else torch.cuda.current_stream(engine.device)
    rc = engine.lib.erpl_mc_correlation(engine._ctx, C.c_void_p(fac.data_ptr()), C.c_void_p(summ.data_ptr()),
                                        None if mask is None else C.c_void_p(mask.data_ptr()), n, C.byref(spec), C.byref(res),
                                        C.c_void_p(corr.ctypes.data), C.c_void_p(rank_corr.ctypes.data),
                                        C.c_void_p(ranks.data_ptr()), C.c_void_p(st.cuda_stream))
    _abi.check(engine.lib, rc, "erpl_mc_correlation")
    return bytes(res), corr.tobytes(), rank_corr.tobytes(), ranks.cpu().numpy().tobytes()


def test_two_calls_give_the_same_bytes(engine):
    rows = [_abi.SUM_RANGE, _abi.SUM_APOGEE_ALT, _abi.SUM_FLIGHT_TIME]
    fac, summ = synthetic(70001, 19, rows, seed=31)
    mask = (np.random.RandomState(32).uniform(size=70001) < 0.1).astype(np.uint8)
    args = (dev(engine, fac), dev(engine, summ), dev(engine, mask), rows)
    first = raw_call(engine, *args)
    assert raw_call(engine, *args) == first
    for other in (300001, 513):                                     # the workspace regrown, then larger than needed
        f2, s2 = synthetic(other, 19, rows, seed=33)
        raw_call(engine, dev(engine, f2), dev(engine, s2), None, rows)
        assert raw_call(engine, *args) == first, other


def test_correlation_is_ordered_behind_the_stream(engine):
    """Inputs produced by torch ops on a side stream that is handed over as hip_stream: the result of the finished inputs."""
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE]
    n = 1 << 18
    fac, summ = synthetic(n, 5, rows, seed=41)
    src_f, src_s = dev(engine, fac), dev(engine, summ)
    want = raw_call(engine, src_f, src_s, None, rows)
    df = torch.full(fac.shape, float("nan"), dtype=torch.float64, device=engine.device)
    ds = torch.full(summ.shape, float("nan"), dtype=torch.float64, device=engine.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=engine.device)
    with torch.cuda.stream(side):
        tmp = src_s
        for _ in range(40):              # some work in front of the copies, all on the side stream
            tmp = tmp * 1.0
        ds.copy_(tmp)
        df.copy_(src_f * 1.0)
        got = raw_call(engine, df, ds, None, rows, stream=side)
    assert got == want


def test_python_layer_refuses_what_the_kernel_cannot_take(engine):
    summ = torch.zeros((16, 8), dtype=torch.float64, device=engine.device)
    fac = torch.zeros((2, 8), dtype=torch.float64, device=engine.device)
    for bad in (fac.cpu(), fac.float(), fac[:, ::2], torch.zeros((2, 9), dtype=torch.float64, device=engine.device),
                torch.zeros((33, 8), dtype=torch.float64, device=engine.device), fac[0]):
        with pytest.raises(ValueError):
            engine.correlation(bad, summ)
    with pytest.raises(ValueError, match="want_ranks"):
        engine.correlation(fac, summ, ranks=False, want_ranks=True)
    with pytest.raises(_abi.ErplError, match="twice"):
        engine.correlation(fac, summ, rows=[1, 1])
    with pytest.raises(ValueError, match="factor names"):
        analysis.drivers(summ, fac, ["only one"], engine=engine)


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def analyzer():
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    return MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)


def host_drivers_check(d, fac, summ, rows):
    """analysis.drivers against NumPy / SciPy on host copies, over the population the outlier filter leaves."""
    bad = analysis.outlier_mask(summ[_abi.SUM_APOGEE_ALT], summ[_abi.SUM_RANGE], summ[_abi.SUM_FLIGHT_TIME])
    ref = reference(fac, summ, bad.astype(np.uint8), rows)
    F = fac.shape[0]
    assert d["n_outliers"] == int(bad.sum()) and d["n_samples"] == int((~bad).sum())
    assert (d["count"], d["n_masked"], d["n_non_finite"]) == (ref["count"], ref["n_masked"], ref["n_non_finite"])
    assert np.array_equal(d["constant"] != 0, ref["constant"])
    close(d["corr"], ref["corr"])
    close(d["rank_corr"], ref["rank_corr"])
    close(d["pearson"], ref["corr"][F:, :F])
    close(d["spearman"], ref["rank_corr"][F:, :F])
    for coef, fit, key in (("src", "r2", "corr"), ("srrc", "r2_rank", "rank_corr")):
        beta, r2, cond, ok = regression(ref[key], F, len(rows), ref["constant"])
        assert ok
        print(f"{coef}: cond(R_ff) = {cond:.3g}")
        close(d[coef], beta, TOL * cond)
        close(d[fit], r2, TOL * cond)
    return ref


def test_device_run_keeps_its_factors_and_names_its_drivers(engine, analyzer):
    rows = [_abi.SUM_RAIL_EXIT_SPEED, _abi.SUM_APOGEE_ALT]
    out = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 8192, precision="f64_fast", keep_factors=True)
    names = out["factor_names"]
    assert tuple(names) == ("position_x", "position_y", "position_z", "velocity_x", "velocity_y", "velocity_z",
                            "attitude_roll", "attitude_pitch", "attitude_yaw", "angular_velocity_x", "angular_velocity_y",
                            "angular_velocity_z", "mass_multiplier", "motor_thrust_multiplier", "motor_mass_flow_multiplier",
                            "wind_speed", "wind_direction", "wind_mean_u", "wind_mean_v")
    assert out["factors"].shape == (len(names), 8192) and out["factors"].dtype == torch.float64 and out["factors"].is_cuda
    d = analysis.drivers(out["summary"], out["factors"], names, status=out["status"], engine=engine, rows=rows)
    assert d["row_names"] == ["rail_exit_speed", "apogee_altitude"] and d["factor_names"] == list(names)
    for k, name in enumerate(names):
        assert bool(d["constant"][k]) == name.startswith("position_"), name      # the default position sigma is 0
    assert d["regression_ok"] and d["rank_regression_ok"]
    host_drivers_check(d, out["factors"].cpu().numpy(), out["summary"].cpu().numpy(), rows)
    for j in range(2):
        assert d["ranking"][j][-3:] == ["position_x", "position_y", "position_z"]
        rho = np.abs(d["spearman"][j, [names.index(k) for k in d["ranking"][j][:-3]]])
        assert np.all(np.diff(rho) <= 0)
    # rail-exit speed follows sqrt(2 L (T / m - g)): more thrust is faster, more mass is slower.  Signs only.
    thrust, mass = names.index("motor_thrust_multiplier"), names.index("mass_multiplier")
    print(f"rail exit speed: spearman thrust {d['spearman'][0, thrust]:+.4f}, mass {d['spearman'][0, mass]:+.4f}, "
          f"r2_rank {d['r2_rank'][0]:.4f}; ranking {d['ranking'][0][:4]}")
    print(f"apogee: r2_rank {d['r2_rank'][1]:.4f}; ranking {d['ranking'][1][:4]}")
    assert d["spearman"][0, thrust] > 0 and d["spearman"][0, mass] < 0
    # the analyzer's method takes the device path on this dict
    d2 = analyzer.drivers(out, rows=rows)
    assert np.array_equal(d2["corr"], d["corr"], equal_nan=True) and d2["ranking"] == d["ranking"]
    # the default call carries no factors
    plain = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, precision="f64_fast")
    assert "factors" not in plain and "factor_names" not in plain


def test_keep_factors_is_refused_on_more_than_one_rank(analyzer, monkeypatch):
    from erpl_monte_carlo_sim_amd import dist, simulator
    monkeypatch.setattr(dist, "world", lambda: (0, 2))

    def no_gpu(*a, **k):
        raise AssertionError("the refusal comes before any work")
    monkeypatch.setattr(simulator, "shared_engine", no_gpu)
    import erpl_monte_carlo_sim_amd.monte_carlo as mcm
    monkeypatch.setattr(mcm, "shared_engine", no_gpu)
    with pytest.raises(ValueError, match="world size"):
        analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 1024, keep_factors=True)


def test_host_run_drivers_and_plot(engine, analyzer, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(plots, "DPI", 60)
    res = analyzer.run_monte_carlo(dict(H.EXAMPLE_IC), 64)
    assert set(res["results"][0]["motor_inputs"]) == {"motor_thrust", "motor_mass_flow_rate"}
    d = analyzer.drivers(res)
    names = d["factor_names"]
    assert "motor_thrust" in names and "motor_mass_flow_rate" in names and "random_seed" not in names
    assert names[0] == "initial_position_offset[0]" and len(names) == 19
    assert d["row_names"] == ["apogee_altitude", "range", "flight_time"] and d["count"] == res["n_samples"] - d["n_non_finite"]
    fac, names2 = analysis.factors_from_results(res["results"])
    assert names2 == names
    summ = analysis.summary_from_results(res["results"])
    ref = reference(fac, summ, None, d["rows"])
    assert d["count"] == ref["count"] and np.array_equal(d["constant"] != 0, ref["constant"])
    close(d["pearson"], ref["corr"][19:, :19])
    close(d["spearman"], ref["rank_corr"][19:, :19])
    thrust = fac[names.index("motor_thrust")]
    assert np.all(thrust > 0) and thrust.min() < thrust.max()
    out_dir = analyzer.plot_drivers(res)
    png = os.path.join(out_dir, "monte_carlo_drivers.png")
    assert os.path.realpath(png).startswith(os.path.realpath(str(tmp_path))) and os.path.getsize(png) > 10000
    fig = plots.drivers_figure(d, "range", top=5)
    assert len(fig.axes[0].patches) == 10                            # spearman and srrc of five factors
