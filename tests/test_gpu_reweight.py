"""erpl_mc_reweight on the device against its host twin (the same header code, itself held to the restatement reweight_ref by
test_reweight_abi.py) - never device against itself alone - and MonteCarloAnalyzer.reweight over flights against a run that
was actually flown under the target law."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import helpers as H
import reweight_cases as RC

pytestmark = pytest.mark.gpu

# 262 145 and 300 001: the grid is capped at 1024 workgroups, a thread takes more than one column
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 70001, 262145, 300001)


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def numpy_of(out):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def on_device(engine, case, pad=0):
    """The case through TrajectoryEngine.reweight; pad > 0: factors and summary sit in wider device matrices (ld = n + pad)."""
    n = case["factors"].shape[1]
    if pad:
        f = torch.full((case["factors"].shape[0], n + pad), -1e300, dtype=torch.float64, device="cuda")
        s = torch.full((_abi.SUMMARY_DIM, n + pad), math.nan, dtype=torch.float64, device="cuda")
        f[:, :n], s[:, :n] = dev(case["factors"]), dev(case["summary"])
        f, s = f[:, :n], s[:, :n]
    else:
        f, s = dev(case["factors"]), dev(case["summary"])
    return numpy_of(engine.reweight(f, case["kinds"], case["law"], s, mask=dev(case["mask"]), rows=case["rows"], extra=dev(case["extra"]),
                                    thresholds=case["thresholds"], quantiles=case["quantiles"], want_weights=True))


def on_host(case):
    return analysis.reweight_host(case["factors"], case["kinds"], case["law"], case["summary"], mask=case["mask"], rows=case["rows"],
                                  extra=case["extra"], thresholds=case["thresholds"], quantiles=case["quantiles"], want_weights=True)


def same_bytes(a, b):
    """Two results of one call: everything, the doubles included, bit for bit."""
    plain = lambda d: {k: v for k, v in d.items() if k not in ("logw", "weights")}
    return (H.same_nested(plain(a), plain(b)) and np.array_equal(RC.bits(a["logw"]), RC.bits(b["logw"]))
            and np.array_equal(a["weights"], b["weights"]))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", RC.VARIANTS)
def test_device_matches_the_host_twin(engine, variant, n):
    case = RC.make_case(variant, n)
    want = on_host(case)
    got = on_device(engine, case)
    RC.compare(got, want, f"{variant}-{n}", scales=RC.mean_scales(case, want["weights"]))
    assert same_bytes(on_device(engine, case), got)                 # a second call: the same bytes in everything


@pytest.mark.parametrize("n", (257, 70001))
def test_a_strided_ld_and_a_stream_of_its_own(engine, n):
    case = RC.make_case("mixed", n)
    want = on_host(case)
    scales = RC.mean_scales(case, want["weights"])
    plain = on_device(engine, case)
    wide = on_device(engine, case, pad=7)
    RC.compare(wide, want, "strided", scales=scales)
    assert same_bytes(wide, plain)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = on_device(engine, case)
    RC.compare(other, want, "stream", scales=scales)
    assert same_bytes(other, plain)


def test_the_kept_outputs_are_optional(engine):
    """Without logw / weights the call keeps both in its own workspace: the same result."""
    case = RC.make_case("extra_row", 1025)
    with_them = on_device(engine, case)
    without = numpy_of(engine.reweight(dev(case["factors"]), case["kinds"], case["law"], dev(case["summary"]), rows=case["rows"],
                                       extra=dev(case["extra"]), thresholds=case["thresholds"], quantiles=case["quantiles"]))
    assert H.same_nested(without, {k: v for k, v in with_them.items() if k not in ("logw", "weights")})


def test_an_empty_support_on_the_device(engine):
    n = 300
    u = np.linspace(0.001, 0.999, n)[None, :].copy()
    summary = np.random.default_rng(3).normal(size=(_abi.SUMMARY_DIM, n))
    case = dict(factors=u, kinds=[RC.U], law=[(0.9995, 1.0)], summary=summary, mask=None, rows=None, extra=None,
                thresholds={_abi.SUM_RANGE: [0.0]}, quantiles=(0.0, 0.5, 1.0))
    got, want = on_device(engine, case), on_host(case)
    RC.compare(got, want, "empty", scales={r: math.nan for r in got["rows"]})
    assert got["count"] == 0 and got["sum_w"] == 0 and math.isnan(got["ess"]) and np.all(np.isneginf(got["logw"])) and not np.any(got["weights"])
    one = dict(case, law=[(u[0, 137] - 1e-9, u[0, 137] + 1e-9)])
    got, want = on_device(engine, one), on_host(one)
    RC.compare(got, want, "one column", scales=RC.mean_scales(one, want["weights"]))
    assert got["count"] == 1 and got["ess"] == 1.0 and got["rows"][_abi.SUM_RANGE]["quantiles"] == [summary[_abi.SUM_RANGE, 137]] * 3


def test_refusals_leave_the_outputs_untouched(engine):
    n = 300
    case = RC.make_case("one_row", n)
    f, s = dev(case["factors"]), dev(case["summary"])
    logw = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    weights = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    res = _abi.ErplReweight()
    C.memset(C.byref(res), 0xA5, C.sizeof(res))
    before = bytes(res)
    lib = engine.lib
    for change, word in (({"n_law": 0}, b"n_law"), ({"s0": -1.0}, b"s[0]"), ({"n_rows": 9}, b"n_rows"), ({"row0": 16}, b"extra"), ({"q0": 2.0}, b"q[0]"),
                         ({"n": 0}, b"n ="), ({"ld": n - 1}, b"ld =")):
        spec = analysis.reweight_spec(case["kinds"], case["law"])
        spec.n_law = change.get("n_law", spec.n_law)
        spec.s[0] = change.get("s0", spec.s[0])
        spec.n_rows = change.get("n_rows", spec.n_rows)
        spec.rows[0] = change.get("row0", spec.rows[0])
        spec.q[0] = change.get("q0", spec.q[0])
        rc = lib.erpl_mc_reweight(engine._ctx, C.byref(spec), C.c_void_p(f.data_ptr()), change.get("ld", n), C.c_void_p(s.data_ptr()), n, None, None,
                                  change.get("n", n), C.byref(res), C.c_void_p(logw.data_ptr()), C.c_void_p(weights.data_ptr()), None)
        assert rc == -1 and word in lib.erpl_mc_last_error(), (change, lib.erpl_mc_last_error())
    torch.cuda.synchronize()
    assert bytes(res) == before and bool((logw == -7.0).all()) and bool((weights == -7).all())
    with pytest.raises(ValueError):
        engine.reweight(f, case["kinds"], case["law"] + [(0.0, 1.0)], s)
    with pytest.raises(ValueError):
        engine.reweight(f.cpu(), case["kinds"], case["law"], s)


# ------------------------------------------------------------------------------------------------ flights
# mass_uncertainty 0.02 -> 0.01 and wind_speed_range [0, 5] -> [3, 5] alone leave the three compared quantities of the unweighted
# flown run inside the bound (0.05, 0.07 and 0.50 of it, measured): the comparison would show nothing.  With the wind also
# known to come from the half-plane the rocket leans into, the mean range moves by more than four bounds.
TARGET = {"mass_uncertainty": 0.01, "wind_speed_range": [3.0, 5.0], "wind_direction_range": [math.pi / 2, 3 * math.pi / 2]}


@pytest.fixture(scope="module")
def flights():
    """The flown run (planar, 4096 flights, design='random', the default table), the same with design='qmc', and a run of 4096
    flights actually flown under the target table with another seed."""
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    make = lambda: MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    mc = make()
    flown = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, seed=2024, planar=True, design="random")
    qmc = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, seed=2024, planar=True, design="qmc")
    direct_mc = make()
    direct_mc.uncertainty_params.update(TARGET)
    direct = direct_mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, seed=777, planar=True, design="random")
    return mc, flown, qmc, direct


def plain_estimates(run, threshold):
    """(value, standard error) of the mean apogee, the mean range and P(range > threshold) over the samples the filter keeps."""
    valid = run["valid_mask"] if "valid_mask" in run else None
    summ = run["summary"]
    if valid is None:
        why = analysis._filter(summ, run.get("status"), None)[2]
        valid = why == 0
    apo, rng = summ[_abi.SUM_APOGEE_ALT][valid].cpu().numpy(), summ[_abi.SUM_RANGE][valid].cpu().numpy()
    m = apo.size
    p = float((rng > threshold).sum()) / m
    return [(apo.mean(), apo.std() / math.sqrt(m)), (rng.mean(), rng.std() / math.sqrt(m)), (p, math.sqrt(p * (1.0 - p) / m))]


def test_reweighted_flights_agree_with_flights_under_the_target_law(flights):
    """Flown: the default table.  Target: mass_uncertainty 0.02 -> 0.01, wind_speed_range [0, 5] -> [3, 5] and
    wind_direction_range [0, 2 pi] -> [pi / 2, 3 pi / 2], an expected ESS share of 0.661 * 0.4 * 0.5 = 0.13.  The means of
    apogee and range and P(range > the flown run's 0.9 quantile), reweighted, against a second run flown under the target
    table: |reweighted - direct| <= 5 sqrt(se_rw^2 + se_direct^2) - a derived bound, 6e-7 per comparison.  Not vacuous: at
    least one of the three, UNWEIGHTED, lies outside that same bound.
    Measured on one MI355X (design='random'): ESS 514 of 3315 kept flights; mean range reweighted 6255 +- 44 m, direct
    6305 +- 17 m, unweighted 5288 m - 0.21 and 4.28 of the bound; P reweighted 0.219 +- 0.018, direct 0.226, unweighted
    0.100 - 0.07 and 1.29 of the bound; mean apogee 0.10 and 0.26 of it."""
    mc, flown, qmc, direct = flights
    why = analysis._filter(flown["summary"], flown["status"], None)[2]
    threshold = float(np.quantile(flown["summary"][_abi.SUM_RANGE][why == 0].cpu().numpy(), 0.9))
    want = plain_estimates(direct, threshold)
    unweighted = plain_estimates(flown, threshold)
    outside = []
    for name, run in (("random", flown), ("qmc", qmc)):
        out = mc.reweight(run, uncertainty=TARGET, rows=["apogee_altitude", "range"], thresholds={"range": [threshold]}, planar=True)
        assert out["primitive_rows"] == [12, 317, 318] and out["warnings"] == [] and math.isclose(out["ess_expected_share"], 0.1323, rel_tol=1e-3)
        apo, rng = out["rows"][_abi.SUM_APOGEE_ALT], out["rows"][_abi.SUM_RANGE]
        got = [(apo["mean"], apo["mean_se"]), (rng["mean"], rng["mean_se"]), (rng["p"][0], rng["p_se"][0])]
        print(f"{name}: ess {out['ess']:.1f} of {out['count'] + out['n_outside']} (share {out['ess_share']:.4f}), threshold {threshold:.3f}")
        for what, (g, g_se), (w, w_se), (u, _) in zip(("mean apogee", "mean range", "P(range > q90)"), got, want, unweighted):
            bound = 5.0 * math.sqrt(g_se * g_se + w_se * w_se)
            print(f"  {what}: reweighted {g:.6g} +- {g_se:.3g}, direct {w:.6g} +- {w_se:.3g}, unweighted {u:.6g}; bound {bound:.3g}")
            assert abs(g - w) <= bound, (name, what, g, w, bound)
            if name == "random":
                outside.append(abs(u - w) > bound)
    assert any(outside), "the unweighted flown run agrees with the target run within the bound: the comparison shows nothing"


def test_a_run_without_a_design_is_refused(flights):
    mc = flights[0]
    joint = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 256, seed=5, planar=True)
    with pytest.raises(ValueError, match="design"):
        mc.reweight(joint, uncertainty=TARGET, planar=True)
    with pytest.raises(ValueError, match="no primitive changes"):
        mc.reweight(flights[1], uncertainty={"mass_uncertainty": 0.02}, planar=True)
