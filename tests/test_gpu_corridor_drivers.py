"""erpl_mc_corridor_drivers on a real MI355X (`pytest -m gpu`) against the NumPy restatement of the definitions in
include/erpl_mc.h (corridor_drivers_ref.restate: plain two-pass formulae row by row, itself held to np.corrcoef and
np.linalg.lstsq by test_corridor_drivers_ref.py).

Bounds.  count, n_*, min, max, constant, regression_ok: exact.  NaN where the contract says NaN.  mean: 1e-12 * mean|x|; std:
1e-12 * std; pearson: 1e-12 absolute (the bar of the other statistics tests).  src and r2: 1e-10 absolute on factor sets whose
correlation matrix has condition number <= 10 - pearson's bound times the condition number with a margin of 10 - and the same
rule, 1e-12 * 10 * cond, where a row's own population has a larger one (corridor_drivers_ref.src_bound).  The worst figures are
printed before they are asserted."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import corridor_drivers_ref as ref
import helpers as H

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1, 1), (257, 300, 5, 21), (1000, 1024, 19, 130), (4099, 4099, 32, 21))


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(engine, x, y, mask, m, regression=True):
    dev = engine.device
    return engine.corridor_drivers(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev),
                                   mask=None if mask is None else torch.from_numpy(mask).to(dev), m=m, regression=regression)


def same_nan(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want))


def worst(got, want):
    """max |got - want| over the places where both are numbers (0.0 where there is none)"""
    both = ~np.isnan(got) & ~np.isnan(want)
    return float(np.max(np.abs(got[both] - want[both]), initial=0.0))


def hold(got, want, what, regression=True):
    """The device's dict against the restatement's, at the bounds of the module docstring."""
    for k in ("m", "n_base", "n_masked", "n_factor_non_finite"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["count"], want["count"]), what
    assert np.array_equal(got["constant"], want["constant"]) and np.array_equal(got["factor_constant"], want["factor_constant"]), what
    for k in ("min", "max", "factor_min", "factor_max"):
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    figures = {}
    for pre in ("", "factor_"):
        assert same_nan(got[pre + "mean"], want[pre + "mean"]) and same_nan(got[pre + "std"], want[pre + "std"]), (what, pre)
        scale = want[pre + "mean_abs"]
        figures[pre + "mean"] = np.nanmax(np.abs(got[pre + "mean"] - want[pre + "mean"]) / np.where(scale > 0, scale, 1.0), initial=0.0)
        figures[pre + "std"] = np.nanmax(np.abs(got[pre + "std"] - want[pre + "std"]) / np.where(want[pre + "std"] > 0, want[pre + "std"], 1.0),
                                         initial=0.0)
    assert same_nan(got["pearson"], want["pearson"]), what
    figures["pearson"] = worst(got["pearson"], want["pearson"])
    if regression:
        assert np.array_equal(got["regression_ok"], want["regression_ok"]), (what, np.flatnonzero(got["regression_ok"] != want["regression_ok"]))
        assert same_nan(got["src"], want["src"]) and same_nan(got["r2"], want["r2"]) and same_nan(got["pivot_min"], want["pivot_min"]), what
        bound = ref.src_bound(np.where(np.isnan(want["cond"]), 10.0, want["cond"]))
        with np.errstate(invalid="ignore"):
            figures["src / bound"] = float(np.nanmax(np.abs(got["src"] - want["src"]) / bound[:, None], initial=0.0))
            figures["r2 / bound"] = float(np.nanmax(np.abs(got["r2"] - want["r2"]) / bound, initial=0.0))
    else:
        assert got["src"] is None and np.isnan(got["r2"]).all() and np.isnan(got["pivot_min"]).all() and not got["regression_ok"].any()
    print(what, {k: f"{v:.3g}" for k, v in figures.items()})
    assert figures["mean"] <= 1e-12 and figures["factor_mean"] <= 1e-12 and figures["std"] <= 1e-12 and figures["factor_std"] <= 1e-12, figures
    assert figures["pearson"] <= 1e-12, figures
    if regression:
        assert figures["src / bound"] <= 1.0 and figures["r2 / bound"] <= 1.0, figures


@pytest.fixture(scope="module")
def cases():
    """The data of every shape and its restatement, computed once."""
    out = {}
    for m, ld, F, R in SHAPES:
        x, y, mask = ref.make_case(m, ld, F, R, seed=11 + m)
        out[m] = (x, y, mask, ref.restate(x, y, mask, m))
    return out


@pytest.mark.parametrize("m,ld,F,R", SHAPES)
def test_against_the_restatement(engine, cases, m, ld, F, R):
    x, y, mask, want = cases[m]
    got = run(engine, x, y, mask, m)
    hold(got, want, f"m = {m}, F = {F}, rows = {R}")
    if F >= 5:
        assert got["count"][ref.ROW_ALL_NAN] == 0 and got["count"][ref.ROW_ONE] == 1
        assert got["constant"][ref.ROW_CONSTANT] and got["constant"][ref.ROW_ZEROS] and got["factor_constant"][2]
        assert np.isnan(got["pearson"][ref.ROW_FACTOR_CONSTANT, 3]) and np.isfinite(got["pearson"][ref.ROW_FACTOR_CONSTANT, 0])
        # the row with as many columns as factors in its regression fails by itself
        big = got["count"] > 3 * F
        assert not got["regression_ok"][ref.ROW_COUNT_F] and got["regression_ok"][big].all() and (want["cond"][big] <= 10.0).all()
        assert np.isfinite(got["pearson"][ref.ROW_COUNT_F, [0, 1]]).all() and np.isnan(got["src"][ref.ROW_COUNT_F]).all()


def test_a_row_with_count_equal_to_the_number_of_factors_fails_alone(engine):
    rng = np.random.default_rng(3)
    F, m = 4, 500
    x = rng.normal(size=(F, m))
    y = x[0] - 2.0 * x[2] + rng.normal(size=(6, m))
    y[3] = np.nan
    y[3, 100:100 + F] = rng.normal(size=F)
    got, want = run(engine, x, y, None, m), ref.restate(x, y, None, m)
    hold(got, want, "count = F")
    assert got["count"][3] == F and got["regression_ok"].tolist() == [True, True, True, False, True, True]
    assert np.isnan(got["src"][3]).all() and np.isnan(got["r2"][3]) and np.isfinite(got["pearson"][3]).all()


def test_an_affine_pair_fails_every_regression_and_keeps_the_correlations(engine):
    x, y, mask = ref.make_case(257, 300, 5, 21, seed=5, affine=True)
    got, want = run(engine, x, y, mask, 257), ref.restate(x, y, mask, 257)
    assert not got["regression_ok"].any() and np.isnan(got["src"]).all() and np.isnan(got["r2"]).all()
    hold(got, want, "affine pair")


def test_same_bytes_twice_for_a_subset_of_rows_and_without_the_regression(engine, cases):
    x, y, mask, want = cases[257]
    a, b = run(engine, x, y, mask, 257), run(engine, x, y, mask, 257)
    keys = ("count", "mean", "std", "min", "max", "r2", "pivot_min", "pearson", "src")
    for k in keys:
        assert same_bits(a[k], b[k]), k
    rows = [3, 7, 20]
    sub = run(engine, x, np.ascontiguousarray(y[rows]), mask, 257)
    for k in keys:
        assert same_bits(sub[k], a[k][rows]), k
    assert np.array_equal(sub["regression_ok"], a["regression_ok"][rows]) and np.array_equal(sub["constant"], a["constant"][rows])
    plain = run(engine, x, y, mask, 257, regression=False)
    assert same_bits(plain["pearson"], a["pearson"])
    hold(plain, ref.restate(x, y, mask, 257, regression=False), "no regression", regression=False)
    # the larger shapes take more than one slice and more than one tile of rows
    x, y, mask, _ = cases[4099]
    a, b = run(engine, x, y, mask, 4099), run(engine, x, y, mask, 4099)
    for k in keys:
        assert same_bits(a[k], b[k]), k


def test_more_rows_than_one_launch_of_the_product_pass_takes(engine):
    """At 131 072 columns (32 slices, two segments) and 32 factors a launch of the product pass takes 52 tiles of 32 rows: 1701
    rows need two.  The rows are 7 rows repeated, so every copy must return the bytes of the first - whatever tile, launch and
    place within a tile it has - and the first seven are held to the restatement."""
    import os
    import subprocess
    exe = os.path.join(H.REPO, "erpl_monte_carlo_sim_amd", "csrc", "erpl_stat_layout_table")
    m, F, R = 131072, 32, 1701
    line = subprocess.run([exe], input=f"cdrv {m} {R} {F} 1\n", capture_output=True, text=True, check=True).stdout.split()
    slices, chunk_tiles = int(line[12]), int(line[13])
    assert slices == 32 and chunk_tiles < (R + 31) // 32 <= 2 * chunk_tiles
    g = torch.Generator(device=engine.device)
    g.manual_seed(4)
    x = torch.randn((F, m), dtype=torch.float64, device=engine.device, generator=g)
    seven = x[:7] * 2.0 - x[7:14] + torch.randn((7, m), dtype=torch.float64, device=engine.device, generator=g)
    seven.masked_fill_(torch.rand((7, m), device=engine.device, generator=g) < 0.3, float("nan"))
    got = engine.corridor_drivers(x, seven.repeat(R // 7, 1))
    assert got["count"].shape == (R,)
    for k in ("count", "mean", "std", "min", "max", "r2", "pivot_min", "pearson", "src"):
        first = got[k][:7]
        assert same_bits(got[k], np.concatenate([first] * (R // 7))), k
    want = ref.restate(x.cpu().numpy(), seven.cpu().numpy())
    hold({k: (v[:7] if isinstance(v, np.ndarray) and v.shape[:1] == (R,) else v) for k, v in got.items()}, want, "two launches")


def test_three_dimensional_values_keep_their_shape(engine, cases):
    x, y, mask, want = cases[257]
    dev = engine.device
    got = engine.corridor_drivers(torch.from_numpy(x).to(dev), torch.from_numpy(y.reshape(3, 7, 300)).to(dev),
                                  mask=torch.from_numpy(mask).to(dev), m=257)
    flat = run(engine, x, y, mask, 257)
    assert got["count"].shape == (3, 7) and got["pearson"].shape == (3, 7, 5) and got["src"].shape == (3, 7, 5)
    assert same_bits(got["pearson"].reshape(21, 5), flat["pearson"]) and same_bits(got["r2"].reshape(21), flat["r2"])


def test_summary_rows_against_erpl_mc_correlation(engine):
    """Rows that are finite everywhere share one population: the call must agree with erpl_mc_correlation(ranks=False)."""
    n, F = 3001, 7
    rng = np.random.default_rng(8)
    x = rng.normal(size=(F, n)) * np.arange(1, F + 1)[:, None] + 10.0
    summ = rng.normal(size=(_abi.SUMMARY_DIM, n))
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
    summ[rows[0]] = 3e4 + 2e3 * x[0] - 1e3 * x[3] + 500.0 * rng.normal(size=n)
    summ[rows[1]] = 1e5 + 7e3 * x[1] + 3e3 * x[0] * x[2] + 1e3 * rng.normal(size=n)
    summ[rows[2]] = 300.0 + 5.0 * x[4] + rng.normal(size=n)
    dev = engine.device
    fx, fs = torch.from_numpy(x).to(dev), torch.from_numpy(summ).to(dev)
    corr = engine.correlation(fx, fs, rows=rows, ranks=False)
    got = engine.corridor_drivers(fx, fs[rows].contiguous())
    assert corr["count"] == n and (got["count"] == n).all() and corr["regression_ok"] and got["regression_ok"].all()
    figures = {"pearson": worst(got["pearson"], corr["pearson"]), "src": worst(got["src"], corr["src"]), "r2": worst(got["r2"], corr["r2"])}
    print("against erpl_mc_correlation", figures)
    assert figures["pearson"] <= 1e-12 and figures["src"] <= 1e-10 and figures["r2"] <= 1e-10
    assert np.linalg.cond(corr["corr"][:F, :F]) <= 10.0


def test_known_answer_the_lead_flips_where_the_effects_cross(engine):
    m, T = 2048, 16
    rng = np.random.default_rng(21)
    x = np.vstack([2.0 * rng.normal(size=m), 0.5 * rng.normal(size=m), rng.normal(size=m)])   # x_1, x_2 and a factor without effect
    a, b, sigma = np.linspace(1.0, 0.0, T), np.linspace(0.0, 4.0, T), 0.3
    y = a[:, None] * x[0] + b[:, None] * x[1] + sigma * rng.normal(size=(T, m))
    dev = engine.device
    out = analysis.corridor_drivers(torch.from_numpy(y[None]).to(dev), torch.from_numpy(x).to(dev), ["x_1", "x_2", "idle"],
                                    channels=["z"], t0=0.0, dt=2.0, engine=engine)
    sd = x.std(axis=1)
    want = ["x_1" if abs(a[k]) * sd[0] > abs(b[k]) * sd[1] else "x_2" for k in range(T)]
    assert out["lead"] == [want] and "x_1" in want and "x_2" in want
    effect = (a * sd[0]) ** 2 + (b * sd[1]) ** 2
    assert np.max(np.abs(out["r2"][0] - effect / (effect + sigma ** 2))) <= 0.05
    assert out["ranking"][0][2] == "idle" and out["time"][-1] == 30.0 and out["share"].shape == (1, T, 3)
    assert np.array_equal(out["share"], out["pearson"] ** 2)


def test_end_to_end_on_captured_flights(engine, tmp_path):
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    cap = int(np.ceil(mc.max_time / 0.005 / 25)) + 4
    kw = dict(stride=25, seed=5, planar=True, capture_bytes=40 * cap * 120 + 119, nodes=16)   # two sub-batches: 40 + 24 samples
    kept = mc.trajectory_corridor(dict(H.EXAMPLE_IC), 64, keep_factors=True, **kw)
    plain = mc.trajectory_corridor(dict(H.EXAMPLE_IC), 64, **kw)
    assert kept["performance"]["sub_batches"] == 2
    assert set(kept) - set(plain) == {"factors", "factor_names"} and set(plain) <= set(kept)
    for k in ("values", "summary"):
        assert same_bits(kept[k].cpu().numpy(), plain[k].cpu().numpy()), k
    assert torch.equal(kept["status"], plain["status"]) and torch.equal(kept["reasons"], plain["reasons"])
    # the factors are those run_monte_carlo_device keeps for the same draws, sub-batch by sub-batch
    parts = [mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), cnt, seed=5 + 1000003 * j, planar=True, keep_factors=True)
             for j, cnt in enumerate((40, 24))]
    assert kept["factor_names"] == parts[0]["factor_names"]
    assert same_bits(kept["factors"].cpu().numpy(), np.concatenate([p["factors"].cpu().numpy() for p in parts], axis=1))
    assert tuple(kept["factors"].shape) == (len(kept["factor_names"]), 64) and kept["factors"].is_cuda

    def against_restatement(captured):
        out = mc.corridor_drivers(captured)
        vals = captured["values"].cpu().numpy()
        want = ref.restate(captured["factors"].cpu().numpy(), vals.reshape(-1, vals.shape[-1]), captured["reasons"].cpu().numpy())
        flat = dict(out)
        for k in ("count", "mean", "std", "min", "max", "r2", "pivot_min", "constant", "regression_ok"):
            flat[k] = out[k].reshape(-1)
        for k in ("pearson", "src"):
            flat[k] = out[k].reshape(-1, out[k].shape[-1])
        hold(flat, want, "captured " + "/".join(captured["channels"]))
        assert out["channels"] == list(captured["channels"]) and out["factor_names"] == captured["factor_names"]
        assert len(out["ranking"]) == vals.shape[0] and len(out["lead"][0]) == vals.shape[1]
        return out, want

    out, _ = against_restatement(kept)
    assert np.array_equal(out["time"], kept["time"])
    trace = mc.impact_point_trace(dict(H.EXAMPLE_IC), 64, stride=25, seed=5, planar=True, capture_bytes=40 * cap * 120 + 119,
                                  nodes=16, keep_factors=True)
    _, want = against_restatement(trace)
    assert np.isnan(trace["values"].cpu().numpy()).any() and len(set(want["count"].tolist())) > 1   # populations differ by node
    # a debris matrix: its rows are (node, fragment) pairs
    deb = mc.debris_footprint(dict(H.EXAMPLE_IC), 64, [(50.0, 10.0), (float("inf"), 0.0)], stride=25, seed=5, planar=True,
                              capture_bytes=40 * cap * 120 + 119, nodes=4, keep_factors=True)
    assert same_bits(deb["factors"].cpu().numpy(), kept["factors"].cpu().numpy())
    dout, _ = against_restatement(deb)
    assert dout["pearson"].shape[:2] == (5, 8) and dout["fragments"] == deb["fragments"]
    assert np.array_equal(dout["time"], np.repeat(deb["time"], 2))
    assert mc.plot_corridor_drivers(dout, save_plots=False) is not None
    with pytest.raises(ValueError, match="keep_factors=True"):
        mc.corridor_drivers(plain)
    mc._create_output_directory = lambda: str(tmp_path)
    fig = mc.plot_corridor_drivers(out, save_plots=False)
    assert fig is not None and len(fig.axes) == 2 * len(out["channels"]) and not list(tmp_path.iterdir())
    mc.plot_corridor_drivers(out, save_plots=True)
    assert (tmp_path / "monte_carlo_corridor_drivers.png").stat().st_size > 1000
