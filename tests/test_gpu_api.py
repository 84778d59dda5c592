"""Drop-in API on the GPU: FlightSimulator.simulate_flight / MonteCarloAnalyzer.run_monte_carlo
used exactly like the reference's example.py, checked against the golden results captured from
the reference itself."""
import numpy as np
import pytest

import erpl_monte_carlo_sim_amd as E
import torch
from erpl_monte_carlo_sim_amd import _abi, flatten

import helpers as H

pytestmark = pytest.mark.gpu


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("key,kind,wind", [("liquid_nowind", "liquid", None), ("solid_nowind", "solid", None),
                                           ("liquid_planar_csv", "liquid", "planar"),
                                           ("liquid_csv_nominal", "liquid", "csv")])
def test_simulate_flight_matches_reference(key, kind, wind):
    idx, arr = H.load_flights("flights_named")
    e = [x for x in idx if x["key"] == key][0]
    s = e["summary"]
    rocket = E.Rocket("Sounding Rocket")
    motor = E.SolidMotor() if kind == "solid" else E.LiquidMotor("Liquid Motor")
    sim = E.FlightSimulator(rocket, motor, E.StandardAtmosphere(), E.WindModel())
    alt, w = (None, None)
    if wind:
        alt, w = H.CSV_ALT.copy(), H.CSV_WIND.copy()
        if wind == "planar":
            w[:, 1] = 0.0
    res = sim.simulate_flight(dict(H.EXAMPLE_IC), w, alt)
    for k in ("time", "position", "velocity", "quaternion", "angular_velocity", "propellant_fraction", "altitude",
              "mass", "moments_of_inertia", "euler_angles", "center_of_mass", "thrust", "drag", "cd", "cl", "cm",
              "cp_location_dynamic", "stability_margin", "angle_of_attack", "sideslip_angle",
              "thrust_curve_time", "thrust_curve_thrust",
              "speed", "apogee_time", "apogee_altitude", "range", "flight_time", "cp_location", "rail_exit_time",
              "rail_exit_position", "rail_exit_velocity", "rail_exit_speed", "rail_exit_euler",
              "rail_exit_angle_of_attack", "rail_exit_sideslip", "wind_at_exit", "initial_conditions",
              "rocket_parameters", "motor_parameters", "simulation_assumptions"):
        assert k in res, k
    n = s["n_steps"] + 1
    assert res["time"].shape == (n,) and res["position"].shape == (3, n) and res["quaternion"].shape == (4, n)
    assert res["time"][0] == 0.0
    assert res["rail_exit_time"] == s["rail_exit_time"]
    assert rel(res["rail_exit_speed"], s["rail_exit_speed"]) < 1e-12
    assert np.allclose(res["rail_exit_position"], s["rail_exit_position"], rtol=1e-12)
    assert np.allclose(res["rail_exit_euler"], s["rail_exit_euler"], rtol=1e-12, atol=1e-15)
    assert np.allclose(res["wind_at_exit"], s["wind_at_exit"], rtol=1e-12, atol=1e-15)
    assert rel(res["flight_time"], s["flight_time"]) < 1e-13
    healthy = key != "liquid_csv_nominal"
    assert rel(res["apogee_altitude"], s["apogee_altitude"]) < (1e-9 if healthy else 1e-6)
    assert rel(res["apogee_time"], s["apogee_time"]) < 1e-12
    if healthy:
        assert rel(res["range"], s["range"]) < 1e-7
        assert res["termination"] == "ground_impact" and res["parachute_deployed"]
    # state history against the reference's (decimated) history
    hi = arr[e["tag"] + "_hist_index"]
    hs = arr[e["tag"] + "_hist_state"]
    ht = arr[e["tag"] + "_hist_time_abs"]
    got = np.vstack([res["position"], res["velocity"], res["quaternion"], res["angular_velocity"],
                     res["propellant_fraction"][None, :]])[:, hi]
    assert np.allclose(res["time"][hi] + res["rail_exit_time"], ht, rtol=1e-13)
    if healthy:
        scale = np.maximum(np.abs(hs), 1e-6)
        assert np.max(np.abs(got - hs) / scale) < 1e-6
    assert np.allclose(res["altitude"], res["position"][2])
    # per-step diagnostic histories (_extract_results) against the reference's
    gd = arr[e["tag"] + "_hist_diag"]
    got_d = np.vstack([res["euler_angles"], res["center_of_mass"][None], res["mass"][None], res["moments_of_inertia"],
                       res["thrust"][None], res["drag"][None], res["cd"][None], res["cl"][None], res["cm"][None],
                       res["cp_location_dynamic"][None], res["stability_margin"][None],
                       res["angle_of_attack"][None], res["sideslip_angle"][None]])[:, hi]
    assert res["mass"].shape == (n,) and res["moments_of_inertia"].shape == (3, n) and res["euler_angles"].shape == (3, n)
    if healthy:
        for r in range(17):
            scale = np.maximum(np.abs(gd[r]), 1e-6 * max(1.0, np.max(np.abs(gd[r]))))
            assert np.max(np.abs(got_d[r] - gd[r]) / scale) < 1e-5, r


@pytest.mark.parametrize("precision", [None, "f64"])
def test_run_monte_carlo_example_config(precision):
    """example.py's Monte Carlo (CSV base profile) with 32 samples: the reference yields
    1 valid / 31 outliers; per-sample scalars match the golden run - with the default build
    (f64_fast since round 4) and with the reference-order kernel."""
    idx, arr = H.load_flights("flights_mc")
    gold = {e["key"][3]: e["summary"] for e in idx if e["key"][:3] == ["liquid", "csv", "seed_i"]}
    mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
    assert mc.precision == "f64_fast"
    if precision:
        mc.precision = precision
    mc.base_altitude_profile, mc.base_wind_profile = H.CSV_ALT, H.CSV_WIND
    out = mc.run_monte_carlo(dict(H.EXAMPLE_IC), n_samples=32)
    assert out["n_samples"] + out["n_outliers"] == 32 and out["n_failed"] == 0
    assert out["n_samples"] == 1 and out["n_outliers"] == 31
    for key in ("apogee_altitude", "range", "flight_time"):
        assert set(out[key]) == {"mean", "std", "min", "max", "percentiles"}
    allr = {r["simulation_id"]: r for r in out["results"] + out["outliers"]}
    for i, s in gold.items():
        r = allr[i]
        assert r["rail_exit_time"] == s["rail_exit_time"]
        assert r["n_steps"] == s["n_steps"]
        if np.isfinite(s["apogee_altitude"]):
            assert rel(r["apogee_altitude"], s["apogee_altitude"]) < 1e-5, i
        else:
            assert not np.isfinite(r["apogee_altitude"])
        assert "parameters" in r and r["parameters"]["random_seed"] == i
    assert all("outlier_reasons" in r for r in out["outliers"])
    v = out["results"][0]
    assert "trajectory" in v and set(v["trajectory"]) == {"time", "altitude", "position"}
    assert v["trajectory"]["position"].shape[1] == 3
    assert "parameter_ranges_observed" in out and "mass_multiplier" in out["parameter_ranges_observed"]


def test_run_monte_carlo_optimized_raises_like_reference():
    """seed-42 stream, 32 samples: 0 valid -> the reference raises ValueError (monte_carlo.py:411-412)."""
    mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
    mc.base_altitude_profile, mc.base_wind_profile = H.CSV_ALT, H.CSV_WIND
    with pytest.raises(ValueError, match="No physically reasonable"):
        mc.run_monte_carlo(dict(H.EXAMPLE_IC), n_samples=32, optimized=True)


def test_run_monte_carlo_fp32_and_synthetic_wind():
    """precision = "f32", SolidMotor, no base profile (100-knot synthetic wind), seed-42 stream: the
    analysis must be exactly what the outlier rules give on the summaries the same engine returns for
    the same samples - or the reference's ValueError when nothing survives them."""
    from erpl_monte_carlo_sim_amd import analysis
    mc = E.MonteCarloAnalyzer(E.Rocket(), E.SolidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
    mc.precision = "f32"
    mc.n_trajectories = 0
    n = 64
    params = mc._generate_parameter_samples_vectorized(n)
    summ, status, traj, lo = mc.run_batch_arrays(dict(H.EXAMPLE_IC), params)
    assert summ.shape == (16, n) and status.shape == (n,) and traj is None and lo == 0
    bad = analysis.outlier_mask(summ[_abi.SUM_APOGEE_ALT], summ[_abi.SUM_RANGE], summ[_abi.SUM_FLIGHT_TIME])
    n_valid = int(n - bad.sum())
    if n_valid == 0:
        with pytest.raises(ValueError, match="No physically reasonable"):
            mc.run_monte_carlo(dict(H.EXAMPLE_IC), n_samples=n, optimized=True)
    else:
        out = mc.run_monte_carlo(dict(H.EXAMPLE_IC), n_samples=n, optimized=True)
        assert out["n_samples"] == n_valid and out["n_outliers"] == n - n_valid and out["n_failed"] == 0
        assert out["performance"]["simulations_per_second"] > 0 and out["performance"]["gpus_used"] == 1
        valid = np.where(~bad)[0]
        assert [r["simulation_id"] for r in out["results"]] == list(valid)
        assert out["apogee_altitude"]["max"] == summ[_abi.SUM_APOGEE_ALT][valid].max()
    # the 100-knot synthetic table really was used, and every sample ended for a reason
    assert np.all((status & 0xFF) <= _abi.END_COAST)


@pytest.mark.parametrize("precision", ["f64", "f64_fast"])
def test_trajectory_split_does_not_change_summaries(precision):
    """run_monte_carlo integrates the samples that carry a trajectory (the first n_trajectories) in a
    small capture batch and the rest through the specialised build.  The reference-order kernel gives the same bits
    either way; in the fp64 throughput build (the default) the capture instantiation fuses a few products differently
    (-ffp-contract=fast), so there the outcomes and step counts are the same and the scalars agree to the rounding
    level times the sample's own error amplification."""
    res = {}
    for n_traj in (0, 5, 40):
        mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
        mc.precision = precision
        mc.base_altitude_profile, mc.base_wind_profile = H.CSV_ALT, H.CSV_WIND
        mc.n_trajectories = n_traj
        params = mc._generate_parameter_samples(40)
        summ, status, traj, lo = mc.run_batch_arrays(dict(H.EXAMPLE_IC), params)
        res[n_traj] = (summ, status)
        assert (traj is None) == (n_traj == 0)
        if traj is not None:
            assert len(traj[0]) == n_traj
    for n_traj in (5, 40):
        assert np.array_equal(res[0][1], res[n_traj][1])
        if precision == "f64":
            assert np.array_equal(res[0][0], res[n_traj][0], equal_nan=True)
        else:
            a, b = res[0][0], res[n_traj][0]
            assert np.array_equal(a[_abi.SUM_STEPS], b[_abi.SUM_STEPS])
            for row, tol in ((_abi.SUM_FIRST_APOGEE_ALT, 1e-9), (_abi.SUM_APOGEE_ALT, 1e-5), (_abi.SUM_RAIL_EXIT_SPEED, 1e-13)):
                same = (a[row] == b[row]) | (np.isnan(a[row]) & np.isnan(b[row]))
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    assert np.all(same | (np.abs(a[row] - b[row]) <= tol * np.abs(a[row]))), row


def test_user_subclass_overriding_model_method_is_refused():
    from erpl_monte_carlo_sim_amd.flatten import UnsupportedModel

    class MyMotor(E.LiquidMotor):
        def get_thrust(self, t, p):      # the kernels would silently ignore this
            return 1.0

    sim = E.FlightSimulator(E.Rocket(), MyMotor(), E.StandardAtmosphere(), E.WindModel())
    with pytest.raises(UnsupportedModel, match="get_thrust"):
        sim.simulate_flight(dict(H.EXAMPLE_IC))


def test_run_monte_carlo_device_large_n():
    """Throughput form (cfg 3-5): on-device dispersions + integration + on-device statistics."""
    mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
    out = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 20000, planar=True)
    assert out["performance"]["precision"] == "f64_fast"     # the parity-preserving build is the default
    assert out["n_samples"] + out["n_outliers"] == 20000
    assert out["n_samples"] > 15000                      # planar dispersions are mostly healthy
    assert 20000 < out["apogee_altitude"]["mean"] < 32000
    assert out["summary"].shape == (16, 20000) and out["status"].shape == (20000,)
    assert sum(out["termination_counts"].values()) == 20000


def test_run_monte_carlo_device_default_build_keeps_the_gate_statistics():
    """run_monte_carlo_device defaults to the fp64 throughput build because its outlier filter and statistics
    consume the reference's apogee_altitude: on reference-faithful (diverging) dispersions its analysis must be
    the gate kernel's - same valid / outlier split up to the 0.15 % of chaotic samples, same statistics - while
    the fp32 build lands elsewhere (documented in DESIGN section 5, asserted here so that it stays visible)."""
    out = {}
    for precision in ("f64", "f64_fast", "f32"):
        mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
        out[precision] = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 30000, seed=77, precision=precision)
    g, f, s = out["f64"], out["f64_fast"], out["f32"]
    assert g["n_samples"] + g["n_outliers"] == 30000
    assert f["n_samples"] == g["n_samples"] and f["n_outliers"] == g["n_outliers"]
    same_apogee = (f["summary"][_abi.SUM_APOGEE_ALT] == g["summary"][_abi.SUM_APOGEE_ALT]) | \
                  (f["summary"][_abi.SUM_APOGEE_ALT].isnan() & g["summary"][_abi.SUM_APOGEE_ALT].isnan()) | \
                  ((f["summary"][_abi.SUM_APOGEE_ALT] - g["summary"][_abi.SUM_APOGEE_ALT]).abs()
                   <= 1e-3 * g["summary"][_abi.SUM_APOGEE_ALT].abs())
    assert float(same_apogee.double().mean()) == 1.0 and bool((f["status"] & 0xFF).eq(g["status"] & 0xFF).all())
    for key in ("apogee_altitude", "flight_time"):
        assert f[key]["mean"] == pytest.approx(g[key]["mean"], rel=1e-6)      # (no sample moves between valid and outlier any more)
        assert f[key]["percentiles"][2] == pytest.approx(g[key]["percentiles"][2], rel=1e-6)
    end_same = float((s["status"] & 0xFF).eq(g["status"] & 0xFF).double().mean())
    print(f"valid: gate {g['n_samples']}, f64_fast {f['n_samples']}, f32 {s['n_samples']}; fp32 same end reason {end_same:.3f}")
    assert end_same < 0.7        # the fp32 build is NOT equivalent here (half of its samples end non-finite)


def test_library_first_then_torch_in_a_fresh_process():
    """The driver may call build() (which loads the library) and smoke() in one interpreter: loading the
    C-ABI library before anything imported torch must still end up on ONE HIP runtime (torch's)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from erpl_monte_carlo_sim_amd import _abi, flatten\n"
            "import numpy as np\n"
            "assert flatten.legacy_streams(np.arange(4, dtype=np.uint32), 'gu').shape == (4, 2)\n"
            "import torch\n"
            "from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine\n"
            "eng = TrajectoryEngine(torch.device('cuda', 0)); eng.close(); print('ok')\n" % root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_chunked_pipeline_and_lazy_results_equal_one_batch():
    """run_monte_carlo builds and submits its samples chunk by chunk (host preparation of chunk i+1 overlaps the
    integration of chunk i) and returns lazy result sequences: same bits as one batch, same dicts as the eager
    list."""
    ref = None
    for chunk in (131072, 300, 97):
        mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
        mc.base_altitude_profile, mc.base_wind_profile = H.CSV_ALT, H.CSV_WIND
        mc.precision = "f64_fast"
        mc.n_trajectories = 3
        mc.CHUNK = chunk
        params = flatten.generate_parameter_arrays(mc.uncertainty_params, 1000)
        summ, status, traj, lo = mc.run_batch_arrays(dict(H.EXAMPLE_IC), params)
        if ref is None:
            ref = (summ, status)
            eager = mc._result_dicts(summ, status, params, traj, lo)
            out = mc.run_monte_carlo(dict(H.EXAMPLE_IC), n_samples=1000)
            assert out["n_samples"] + out["n_outliers"] == 1000
            both = {r["simulation_id"]: r for r in out["results"] + out["outliers"]}
            from erpl_monte_carlo_sim_amd.results import _same_record
            for i in (0, 1, 2, 3, 500, 999):      # incl. the samples that carry a trajectory
                a, b = dict(both[i]), dict(eager[i])
                a.pop("outlier_reasons", None)
                assert _same_record(a, b), i
            assert "trajectory" in both[0] and "trajectory" not in both[3]
        else:
            assert np.array_equal(summ, ref[0], equal_nan=True) and np.array_equal(status, ref[1]), chunk


_THREE_DEEP_CODE = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import erpl_monte_carlo_sim_amd as E
from erpl_monte_carlo_sim_amd import flatten
from erpl_monte_carlo_sim_amd.simulator import shared_engine
import helpers as H
res = []
for chunk in (131072, 97, 97):
    mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
    mc.base_altitude_profile, mc.base_wind_profile = H.CSV_ALT, H.CSV_WIND
    mc.precision = "f64_fast"
    mc.n_trajectories = 3
    mc.CHUNK = chunk
    assert shared_engine(mc.device).get_overlap() == 3
    params = flatten.generate_parameter_arrays(mc.uncertainty_params, 1000)
    res.append(mc.run_batch_arrays(dict(H.EXAMPLE_IC), params)[:2])
for summ, status in res[1:]:
    bad = np.where(~(((summ == res[0][0]) | (np.isnan(summ) & np.isnan(res[0][0]))).all(axis=0) & (status == res[0][1])))[0]
    assert bad.size == 0, ("samples differing from one batch", bad.size, bad[:10].tolist())
print("ok")
"""


def test_chunked_pipeline_three_deep_in_a_fresh_process():
    """The chunked pipeline at the HIP runtime's default of four hardware queues (GPU_MAX_HW_QUEUES=4, which the package
    leaves alone: three batches in flight, no lane adoption) - the depth of any process that sets the variable or starts
    torch.cuda before importing the package.  Eleven 97-sample chunks retire batches while later ones are prepared: the
    inputs of a retired batch must not go back to the allocator before that batch has finished (they were, once, and a
    worker's upload of the next chunk overwrote them: whole chunks came back with other samples' flights)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _THREE_DEEP_CODE % {"root": root}], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, GPU_MAX_HW_QUEUES="4"))
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_run_monte_carlo_device_sub_batches():
    """run_monte_carlo_device splits its samples into sub-batches handed to erpl_mc_submit_batch; the draws of a
    sub-batch depend on (seed, rank, index of the sub-batch) only."""
    mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
    mc.DEVICE_CHUNK = 4096
    a = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 10000, seed=5)
    b = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 10000, seed=5)
    assert a["performance"]["sub_batches"] == 3
    assert torch.equal(a["status"], b["status"])
    assert bool(((a["summary"] == b["summary"]) | (a["summary"].isnan() & b["summary"].isnan())).all())
    assert a["n_samples"] + a["n_outliers"] == 10000 and sum(a["termination_counts"].values()) == 10000
    mc.DEVICE_CHUNK = 1 << 20
    c = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, seed=5)      # = the first sub-batch of the runs above
    assert torch.equal(c["status"], a["status"][:4096])
