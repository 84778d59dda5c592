"""erpl_mc_corridor_bands_weighted on the device against its host twin (the same header code, itself held to the restatement
corridor_w_ref by test_corridor_w_ref.py) - never device against itself alone - against erpl_mc_reweight and
erpl_mc_corridor_bands where they state the same thing, captured runs flown from a design, and
MonteCarloAnalyzer.reweighted_corridor over flights against a corridor that was actually flown under the target law."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import corridor_w_cases as CW
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def on_device(engine, case, values=None):
    v = dev(case["values"]) if values is None else values
    return engine.corridor_bands_weighted(v, dev(case["weights"]), mask=dev(case["mask"]), quantiles=case["quantiles"],
                                          thresholds=case["thresholds"], m=case["m"])


def on_host(case):
    return analysis.bands_weighted_host(case["values"], case["weights"], mask=case["mask"], quantiles=case["quantiles"],
                                        thresholds=case["thresholds"], m=case["m"])


@pytest.mark.parametrize("name", list(CW.CASES))
def test_device_matches_the_host_twin(engine, name):
    case = CW.CASES[name]
    got, want = on_device(engine, case), on_host(case)
    CW.compare(got, want, case, name)
    assert CW.same_bytes(on_device(engine, case), got)      # a second call: the same bytes in everything


def test_a_strided_ld_a_subset_of_the_rows_and_a_stream_of_its_own(engine):
    """The record of a row depends on that row, the mask, the weights and the spec alone."""
    case = CW.CASES["m257"]
    C_, T, ld = case["values"].shape
    m = case["m"]
    plain = on_device(engine, case)
    # another leading dimension, the padding poisoned differently
    wide = np.full((C_, T, ld + 11), -7e299)
    wide[:, :, :m] = case["values"][:, :, :m]
    assert CW.same_bytes(on_device(engine, case, dev(wide)), plain)
    # channel 1 alone, as channel 0 of its own call, with channel 1's thresholds
    sub = dict(case, values=np.ascontiguousarray(case["values"][1:2]), thresholds=[case["thresholds"][1]])
    alone = on_device(engine, sub)
    for k, v in plain.items():
        if isinstance(v, np.ndarray):
            assert v[1:2].tobytes() == alone[k].tobytes(), k
    # node 1 of both channels
    node = dict(case, values=np.ascontiguousarray(case["values"][:, 1:2]))
    one = on_device(engine, node)
    for k, v in plain.items():
        if isinstance(v, np.ndarray):
            assert np.ascontiguousarray(v[..., 1:2]).tobytes() == one[k].tobytes(), k
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = on_device(engine, case)
    assert CW.same_bytes(other, plain)


def test_cross_call_identity_with_reweight(engine):
    """A matrix row that is also erpl_mc_reweight's `extra` row, with the weights and the mask of that call: sum_w, every
    quantile and every exceed_w are the same bits."""
    import reweight_cases as RC
    n = 1025
    case = RC.make_case("extra_row", n)
    rng = np.random.default_rng(11)
    extra = np.round(rng.normal(size=n) * 20.0) / 4.0
    extra[::50] = rng.choice([0.0, -0.0], size=len(extra[::50]))
    mask = (rng.uniform(size=n) < 0.1).astype(np.uint8)
    qs, thr = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0), [0.0, -0.0, 2.5, 100.0]
    rw = engine.reweight(dev(case["factors"]), case["kinds"], case["law"], dev(case["summary"]), mask=dev(mask), rows=[_abi.RW_ROW_EXTRA],
                         extra=dev(extra), thresholds={_abi.RW_ROW_EXTRA: thr}, quantiles=qs, want_weights=True)
    values = np.full((1, 2, n + 3), math.nan)
    values[0, 0, :n], values[0, 1, :n] = rng.normal(size=n), extra
    got = engine.corridor_bands_weighted(dev(values), rw["weights"], mask=dev(mask), quantiles=qs, thresholds=[thr], m=n)
    row = rw["rows"][_abi.RW_ROW_EXTRA]
    assert rw["sum_w"] > 0 and int(got["sum_w"][0, 1]) == rw["sum_w"] and got["max_w"] == rw["max_w"] and got["Q"] == rw["Q"]
    assert np.array_equal(CW.bits(got["quantiles"][0, :, 1]), CW.bits(row["quantiles"]))
    assert got["exceed_w"][0, :, 1].tolist() == row["exceed_w"]
    assert int(got["count"][0, 1]) == rw["count"] - rw["n_zero"]
    assert CW.close(got["mean"][0, 1], row["mean"], RC.mean_scales(dict(case, rows=[_abi.RW_ROW_EXTRA], extra=extra),
                                                                   rw["weights"].cpu().numpy())[_abi.RW_ROW_EXTRA])
    for k in ("var", "std", "mean_se"):
        assert CW.close(got[k][0, 1], row[k]), k
    assert CW.close(got["p"][0, :, 1], row["p"]) and CW.close(got["p_se"][0, :, 1], row["p_se"])
    assert CW.close(got["ess"][0, 1], rw["ess"])


@pytest.mark.parametrize("name", ("m63", "m257", "m4099"))
def test_constant_weights_against_the_unweighted_bands(engine, name):
    """Every W = 2^Q: count, min and max are erpl_mc_corridor_bands' on the same matrix, every quantile the inverted_cdf order
    statistic of the row."""
    case = CW.CASES[name]
    m = case["m"]
    v, mask = dev(case["values"]), dev(case["mask"])
    w = torch.full((m,), 1 << CW.q_bits(m), dtype=torch.int64, device="cuda")
    got = engine.corridor_bands_weighted(v, w, mask=mask, quantiles=case["quantiles"], m=m)
    flat = engine.corridor_bands(v, mask, quantiles=case["quantiles"], m=m)
    assert np.array_equal(got["count"], flat["count"]) and got["n_counted"] == flat["n_counted"]
    for k in ("min", "max"):
        assert np.array_equal(got[k], flat[k], equal_nan=True), k
    open_ = np.ones(m, dtype=bool) if case["mask"] is None else case["mask"] == 0
    C_, T = case["values"].shape[:2]
    for c in range(C_):
        for k in range(T):
            x = case["values"][c, k, :m]
            x = x[open_ & np.isfinite(x)]
            want = np.quantile(x, case["quantiles"], method="inverted_cdf") if len(x) else np.full(len(case["quantiles"]), math.nan)
            assert np.array_equal(got["quantiles"][c, :, k], want, equal_nan=True), (c, k)


def test_a_bad_weight_in_a_masked_column_is_refused_and_nothing_is_written(engine):
    case = CW.CASES["m257"]
    m = case["m"]
    w, mask = case["weights"].copy(), case["mask"].copy()
    w[200], mask[200] = (1 << CW.q_bits(m)) + 1, 1
    w[230] = -1
    spec = analysis.bands_weighted_spec(2, 2, case["quantiles"], case["thresholds"])
    rows = (_abi.ErplBandsWRow * 4)()
    res = _abi.ErplBandsWResult()
    C.memset(rows, 0xA5, C.sizeof(rows))
    C.memset(C.byref(res), 0xA5, C.sizeof(res))
    before = bytes(rows), bytes(res)
    v, wd, md = dev(case["values"]), dev(w), dev(mask)
    rc = engine.lib.erpl_mc_corridor_bands_weighted(engine._ctx, C.c_void_p(v.data_ptr()), C.c_void_p(md.data_ptr()), C.c_void_p(wd.data_ptr()),
                                                    m, v.shape[2], C.byref(spec), C.cast(rows, C.c_void_p), C.byref(res), None)
    msg = engine.lib.erpl_mc_last_error().decode()
    assert rc == -1 and "weights[200]" in msg and "2^52" in msg, msg
    assert (bytes(rows), bytes(res)) == before
    with pytest.raises(ValueError, match="weights"):
        engine.corridor_bands_weighted(v, wd.to(torch.int32), mask=md, m=m)
    with pytest.raises(ValueError, match="weights"):
        engine.corridor_bands_weighted(v, wd.cpu(), mask=md, m=m)


# ------------------------------------------------------------------------------------------------ captured runs from a design
def make_analyzer():
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    return MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)


def test_a_captured_run_flies_the_design_of_the_device_run():
    """The same seed and n_samples: the summary of the capturing run is run_monte_carlo_device's bit for bit (precision 'f64') in
    every entry that is a number, NaN where it has a NaN - as everywhere the suite compares the summary of a capturing run with
    that of a plain one: the capture instantiation of the flight kernel need not give a NaN the sign and payload the plain
    launch gives it (measured on this run: 7 of 4800 entries, rows 10 and 14, NaN on both sides with other bits).  Two values
    of capture_bytes, both capturing, give the same bytes, NaNs included.  The dict carries the design entry of a device run."""
    mc = make_analyzer()
    n, stride = 300, 25
    cap = int(np.ceil(mc.max_time / 0.005 / stride)) + 4
    kw = dict(stride=stride, seed=31, precision="f64", planar=True, nodes=9, channels=("z", "downrange"), design="random")
    whole = mc.trajectory_corridor(dict(H.EXAMPLE_IC), n, **kw)
    cut = mc.trajectory_corridor(dict(H.EXAMPLE_IC), n, capture_bytes=128 * cap * 120 + 7, **kw)
    run = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), n, seed=31, precision="f64", planar=True, design="random")
    torch.cuda.synchronize()
    assert whole["performance"]["sub_batches"] == 1 and cut["performance"]["sub_batches"] == 3
    assert whole["design"] == run["design"] == {"kind": "random", "seed": 31, "block": n, "replicates": 1}
    same = lambda a, b: a.shape == b.shape and bool((a.view(torch.int64) == b.view(torch.int64)).all())
    a, b = whole["summary"], run["summary"]
    assert a.shape == b.shape and bool(((a.view(torch.int64) == b.view(torch.int64)) | (a.isnan() & b.isnan())).all())
    assert torch.equal(whole["status"], run["status"])
    assert same(cut["summary"], whole["summary"]) and same(cut["values"], whole["values"])
    joint = mc.trajectory_corridor(dict(H.EXAMPLE_IC), 64, **dict(kw, design=None))
    assert "design" not in joint
    with pytest.raises(ValueError, match="design"):
        mc.reweighted_corridor(joint, uncertainty={"mass_uncertainty": 0.01}, planar=True)


# ------------------------------------------------------------------------------------------------ flights
# the set-up of test_gpu_reweight.py: its TARGET table, 4096 planar flights, design='random', seed 2024; direct run seed 777
TARGET = {"mass_uncertainty": 0.01, "wind_speed_range": [3.0, 5.0], "wind_direction_range": [math.pi / 2, 3 * math.pi / 2]}


def test_reweighted_corridor_agrees_with_a_corridor_flown_under_the_target_law(tmp_path):
    """Flown: the default table.  Target: TARGET.  At every (channel, node) whose weighted count is the whole kept population:
    |reweighted mean - direct mean| <= 5 sqrt(mean_se^2 + se_direct^2), se_direct = std / sqrt(count) of the unweighted bands of
    the run flown under the target table - the derived bound of test_gpu_reweight.py.  Not vacuous: at one node or more the
    UNWEIGHTED flown mean lies outside that same bound.
    Measured on one MI355X: 3315 kept flights, 761 inside the target's support with a weight, ess 514.3; with hold all 18 rows
    have the whole population and every one is inside the bound, the largest at 0.32 of it (z at 225 s: 2.46 +- 0.42 against
    3.20 +- 0.20); mean downrange at 150 s reweighted 6222 +- 43 m, direct 6269 +- 16 m, unweighted 5150 m - 0.20 and 4.9 of
    the bound; the unweighted mean is outside at the 8 downrange rows from 37.5 s on (DESIGN.md 8.23 has the table)."""
    mc = make_analyzer()
    kw = dict(stride=25, planar=True, nodes=9, hold=True, channels=("z", "downrange"), design="random")
    flown = mc.trajectory_corridor(dict(H.EXAMPLE_IC), 4096, seed=2024, **kw)
    direct_mc = make_analyzer()
    direct_mc.uncertainty_params.update(TARGET)
    direct = direct_mc.trajectory_corridor(dict(H.EXAMPLE_IC), 4096, seed=777, **kw)
    out = mc.reweighted_corridor(flown, uncertainty=TARGET, planar=True, thresholds={0: [1000.0]})
    assert out["primitive_rows"] == [12, 317, 318] and math.isclose(out["ess_expected_share"], 0.1323, rel_tol=1e-3)
    whole = out["count"] - out["n_zero"]      # the flights the filter keeps, inside the target's support, with a weight
    print(f"ess {out['ess']:.1f} of {out['count'] + out['n_outside']} kept flights (share {out['ess_share']:.4f}), {whole} with a weight; "
          f"warnings {out['warnings']}")
    assert whole >= 100
    compared, outside = 0, []
    for name in out["channels"]:
        rew, fl, dr = out[name]["reweighted"], out[name]["flown"], direct[name]
        for k in range(len(out["time"])):
            if rew["count"][k] != whole:
                continue
            g, g_se = rew["mean"][k], rew["mean_se"][k]
            w, w_se = dr["mean"][k], dr["std"][k] / math.sqrt(dr["count"][k])
            bound = 5.0 * math.sqrt(g_se * g_se + w_se * w_se)
            print(f"  {name} t = {out['time'][k]:.1f}: reweighted {g:.6g} +- {g_se:.3g}, direct {w:.6g} +- {w_se:.3g}, "
                  f"unweighted {fl['mean'][k]:.6g}; bound {bound:.3g}; ess {rew['ess'][k]:.1f}")
            assert abs(g - w) <= bound, (name, k, g, w, bound)
            compared += 1
            outside.append(abs(fl["mean"][k] - w) > bound)
    assert compared >= 4, compared
    assert any(outside), "the unweighted flown corridor agrees with the target corridor within the bound: the comparison shows nothing"
    # the Python layer on top: the figure and its JSON
    from erpl_monte_carlo_sim_amd import plots

    class Saver:
        def _create_output_directory(self):
            return str(tmp_path)

    assert plots.plot_reweighted_corridor(Saver(), out) == str(tmp_path)
