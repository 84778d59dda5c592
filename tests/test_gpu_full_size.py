"""Full-size GPU tests: BASELINE config 5's per-GPU share (10 M samples / 8 GPUs = 1.25 M: CSV base
wind + parachute-deploy event + per-GPU compaction) and the N > 1 path with the GPU engine as the
per-rank runner (two processes on one GPU, gloo)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, flatten, models, sampling

import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(a, b):
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = np.abs(a - b) / np.abs(b)
    return np.where(same, 0.0, np.where(np.isnan(e), np.inf, e))


@pytest.mark.parametrize("precision", ["f32", "f64_fast"])
def test_config5_share_csv_wind_parachute_compaction(oracle, precision):
    """BASELINE configs[4] per-GPU share in both throughput builds.  The fp64 one keeps the reference's
    outcome (98 % of these planar flights land under the parachute); in fp32 a fifth of them blows up
    during the tumbling descent (stall model + destabilising yaw term) and ends non-finite
    instead - the numbers below are what each build delivers, asserted so that they cannot drift silently.

    1.25 M samples, CSV base profile (K = 6) + per-sample AR(1) + uniform offset, flights to the ground
    under the parachute latch (simulator.py:366-377), step-chunked launches with compaction
    (erpl_mc_set_chunk(2048)).  The oracle cannot integrate that many, so the full-size run is checked
    through size-independent properties, and a 256-sample subset against the oracle incl. the parachute
    flag and the landing."""
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch, TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    n = 1_250_000
    rocket, motor, wm = models.Rocket(), models.LiquidMotor(), models.WindModel()
    cfg = H.make_config("liquid")
    eng.set_config(cfg)
    prec = _abi.PRECISIONS[precision]
    fp64 = precision != "f32"
    db = sampling.synthetic_dispersions(n, rocket, motor, wm, H.EXAMPLE_IC, eng.device, precision=prec, seed=55,
                                        planar=True, base_altitude_profile=H.CSV_ALT, base_wind_profile=H.CSV_WIND, engine=eng)
    try:
        eng.set_chunk(2048)
        s0, t0 = (x.clone() for x in eng.run(db))
        eng.set_chunk(0)
        eng.set_launch(256, 700, 8)
        s1, t1 = eng.run(db)
        torch.cuda.synchronize()
        # compaction / launch geometry do not change a bit
        assert torch.equal(t0, t1) and bool(((s0 == s1) | (s0.isnan() & s1.isnan())).all())
        del s1, t1
        # sample independence: a strided sub-batch alone reproduces its rows
        eng.set_launch(64, 0, 1)
        eng.set_chunk(2048)
        idx = torch.arange(11, n, 4099, device=eng.device)
        sub = DeviceBatch(db.ic[:, idx].contiguous(), db.rocket[:, idx].contiguous(), db.motor[:, idx].contiguous(),
                          db.alt_grid, db.wind[:, :, idx].contiguous(), prec)
        s2, t2 = eng.run(sub)
        torch.cuda.synchronize()
        assert torch.equal(t2, t0[idx]) and bool(((s2 == s0[:, idx]) | (s2.isnan() & s0[:, idx].isnan())).all())
    finally:
        eng.set_launch(64, 0, 1)
        eng.set_chunk(0)
    summ, status = s0.cpu().numpy(), t0.cpu().numpy()
    reason = status & 0xFF
    chute = (status & _abi.ST_CHUTE) != 0
    assert np.all(reason <= _abi.END_COAST) and np.sum(np.bincount(reason, minlength=5)) == n
    landed = reason == _abi.END_GROUND
    print(f"cfg-5 {precision} share end reasons:", {k: int(np.sum(reason == v)) for k, v in
                                       (("max_time", 0), ("ground", 1), ("altitude_100km", 2), ("coast", 3))},
          "parachute latched:", int(chute.sum()), "NaN:", int(((status & _abi.ST_NAN) != 0).sum()))
    # planar dispersions reach apogee healthy; most come down to the parachute altitude and land under it, near the
    # 0.5 m threshold, slowly (the descent tumbles - stall model + destabilising yaw term - and part of the
    # samples blow up there instead: SURVEY fact 5)
    assert landed.mean() > (0.97 if fp64 else 0.75)
    assert chute[landed].mean() > 0.99
    ok = landed & chute
    assert np.all(summ[_abi.SUM_IMPACT_Z][ok] <= 0.5) and np.all(summ[_abi.SUM_FINAL_VZ][ok] <= 0)
    assert np.median(summ[_abi.SUM_FINAL_VZ][ok]) == pytest.approx(-7.8, abs=0.5)      # -7.78 m/s
    assert 20000 < np.median(summ[_abi.SUM_APOGEE_ALT][ok]) < 32000
    assert np.all(summ[_abi.SUM_FLIGHT_TIME] <= cfg.max_time + 2 * cfg.dt_initial)
    assert np.array_equal((status & _abi.ST_NAN) != 0, np.isnan(summ[_abi.SUM_APOGEE_ALT]))
    fin = np.isfinite(summ[_abi.SUM_APOGEE_ALT]) & np.isfinite(summ[_abi.SUM_FIRST_APOGEE_ALT])
    assert np.all(summ[_abi.SUM_APOGEE_ALT][fin] >= summ[_abi.SUM_FIRST_APOGEE_ALT][fin])
    # the parachute latch can only be set below the deployment altitude on the way down: every latched sample came down
    assert np.all((status[chute] & _abi.ST_APOGEE_LATCHED) != 0)
    # 256-sample subset against the oracle
    pick = np.sort(np.random.RandomState(5).choice(n, 256, replace=False))
    tp = torch.as_tensor(pick, device=eng.device)
    hb = flatten.HostBatch(len(pick), db.k_wind)
    hb.ic = db.ic[:, tp].cpu().numpy(); hb.rocket = db.rocket[:, tp].cpu().numpy(); hb.motor = db.motor[:, tp].cpu().numpy()
    hb.alt_grid = db.alt_grid.cpu().numpy(); hb.wind = db.wind[:, :, tp].double().cpu().numpy()
    osum, ostat = oracle.run_batch(cfg, hb)
    g_s, g_t = summ[:, pick], status[pick]
    both = ((ostat & 0xFF) == _abi.END_GROUND) & ((g_t & 0xFF) == _abi.END_GROUND)
    print(f"cfg-5 {precision} subset: oracle landed {np.mean((ostat & 0xFF) == _abi.END_GROUND):.3f}, fp32 agrees on {both.sum()} of 256")
    assert both.mean() > (0.96 if fp64 else 0.72)   # measured 0.98 / 0.77: the fp32 descent leaves the fp64 solution
    if fp64:
        assert np.array_equal(g_t & 0xFF, ostat & 0xFF)
        assert np.mean(relerr(g_s[_abi.SUM_APOGEE_ALT], osum[_abi.SUM_APOGEE_ALT]) <= 1e-3) == 1.0
        assert np.array_equal(g_s[_abi.SUM_STEPS][both], osum[_abi.SUM_STEPS][both])
    assert np.array_equal((g_t[both] & _abi.ST_CHUTE) != 0, (ostat[both] & _abi.ST_CHUTE) != 0)
    assert np.max(relerr(g_s[_abi.SUM_APOGEE_ALT][both], osum[_abi.SUM_APOGEE_ALT][both])) < (1e-9 if fp64 else 1e-3)
    assert np.mean(relerr(g_s[_abi.SUM_FIRST_APOGEE_ALT], osum[_abi.SUM_FIRST_APOGEE_ALT]) <= 1e-3) >= 0.97
    assert np.median(relerr(g_s[_abi.SUM_FLIGHT_TIME][both], osum[_abi.SUM_FLIGHT_TIME][both])) < 1e-2
    assert np.array_equal(g_s[_abi.SUM_RAIL_EXIT_TIME], osum[_abi.SUM_RAIL_EXIT_TIME])
    eng.close()


_RANK_CODE = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
import torch.distributed as td
td.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
import erpl_monte_carlo_sim_amd as E
import helpers as H
mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), device="cuda:0", verbose=False)
mc.base_altitude_profile, mc.base_wind_profile = H.CSV_ALT, H.CSV_WIND
mc.n_trajectories = 3
calls = []
import erpl_monte_carlo_sim_amd.flatten as F
orig = F.dispersed_batch
def counting(*a, **k):
    hb = orig(*a, **k)
    calls.append(hb.n)
    return hb
F.dispersed_batch = counting
n = int(os.environ["ERPL_TEST_N"])
params = mc._generate_parameter_samples(n)
summ, status, traj, lo = mc.run_batch_arrays(dict(H.EXAMPLE_IC), params)
np.savez(os.environ["ERPL_TEST_OUT"] + f".{td.get_rank()}.npz", summ=summ, status=status, calls=np.array(calls), lo=lo,
         n_traj=0 if traj is None else len(traj[0]))
td.barrier()
td.destroy_process_group()
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("n", [37, 2])
def test_two_ranks_with_the_gpu_engine(tmp_path, n):
    """The N > 1 path end to end with the real engine: two FRESH processes (started before anything here
    touches the GPU in them), both on cuda:0, gloo backend, each building only its own shard on the host and
    integrating it with the HIP kernels through MonteCarloAnalyzer.run_batch_arrays -> dist.run_local_shard;
    the gathered [16, n] block must equal a single-process GPU run bit for bit on both ranks.  (RCCL itself
    needs one GPU per rank and is exercised only by the driver's multi-GPU bench.)"""
    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2",
                   ERPL_TEST_N=str(n), ERPL_TEST_OUT=out, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, "-c", _RANK_CODE % {"root": ROOT}], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    import erpl_monte_carlo_sim_amd as E
    mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), verbose=False)
    mc.base_altitude_profile, mc.base_wind_profile = H.CSV_ALT, H.CSV_WIND
    mc.n_trajectories = 3
    ref_s, ref_t, _, _ = mc.run_batch_arrays(dict(H.EXAMPLE_IC), mc._generate_parameter_samples(n))
    per = -(-n // 2)
    for r in range(2):
        z = np.load(out + f".{r}.npz")
        assert np.array_equal(z["summ"], ref_s, equal_nan=True), r
        assert np.array_equal(z["status"], ref_t), r
        # host preparation is proportional to n / world: the shard's samples and nothing else are built on this rank
        # (in two calls when the shard holds trajectory-carrying samples: the capture batch and the rest)
        assert int(np.sum(z["calls"])) == (per if r == 0 else n - per) and len(z["calls"]) <= 2, (r, z["calls"])
        assert int(z["lo"]) == r * per
        assert int(z["n_traj"]) == (min(3, per) if r == 0 else max(0, min(3, n) - per))


_RCCL_CODE = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
import torch.distributed as td
torch.cuda.set_device(0)
td.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
import erpl_monte_carlo_sim_amd as E
from erpl_monte_carlo_sim_amd import dist, _abi
import helpers as H
mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), device="cuda:0", verbose=False)
mc.n_trajectories = 0
out = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 5000, planar=True)       # ws == 1: no collective inside
summ, status = out["summary"], out["status"]
assert summ.is_cuda and status.is_cuda
g_s, g_t = dist.all_gather_summaries(summ, status, 5000, force_collective=True)   # RCCL all_gather_into_tensor on device buffers
torch.cuda.synchronize()
assert g_s.is_cuda and torch.equal(g_t, status) and bool(((g_s == summ) | (g_s.isnan() & summ.isnan())).all())
print("rccl-ok", td.get_backend(), tuple(g_s.shape))
td.destroy_process_group()
"""


def test_rccl_one_rank_group_runs_the_gather_on_device_buffers():
    """RCCL needs one GPU per rank, so on a one-GPU box only a ONE-rank "nccl" group can run: it still loads
    RCCL, creates the communicator on the device and pushes the [16, n] / [n] device tensors of a real run
    through all_gather_into_tensor - the collective `dist.all_gather_summaries` issues at N > 1."""
    port = _free_port()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", _RCCL_CODE % {"root": ROOT}], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "rccl-ok nccl (16, 5000)" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("mode", ["weak", "strong"])
def test_bench_two_ranks_on_one_gpu(tmp_path, mode):
    """bench.py's own N > 1 pipeline - side stream waiting on ticket i, asynchronous gathers, rotating output
    buffers, the self-check that the gathered block of a rank equals its results - exactly as the driver will
    launch it on an 8-GPU node, here with two ranks on the one GPU and gloo instead of RCCL (RCCL refuses two
    ranks on one device; ERPL_BENCH_BACKEND exists for this rehearsal only).  Two FRESH child processes, started
    before anything in them touches the GPU.  `strong`: --total-samples splits a fixed sample count over the ranks
    (BASELINE configs[3]'s 1 048 576 over 1 / 2 / 4 / 8 GPUs the moment a node exists)."""
    import json
    n_rank = 16384
    extra = ["--total-samples", str(2 * n_rank)] if mode == "strong" else ["--samples-per-gpu", str(n_rank)]
    # typed exactly as the driver types the N = 1 run, with --gpus 2: bench.py starts its two ranks itself
    # (fresh children, the launching process never touches the GPU) and relays rank 0's line
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--full",
           "--cpu-seconds", "0", "--no-parity", "--no-cfg5", "--no-api", "--dump-outputs", str(tmp_path / "dump")] + extra
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(ERPL_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    outs = [(r.stdout, r.stderr)]
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1   # rank 0 prints the ONE line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["warmup"] == 1 and d["value"] > 0 and d["dtype"] == "f64_fast"
    assert d["scaling"] == mode and d["config"]["samples_per_gpu"] == n_rank
    assert d["cpu_baseline"] is None and "f32" in d and d["f32"]["value"] > 0
    # value = the samples of BOTH ranks per second of the slowest rank
    assert d["value"] == pytest.approx(2 * n_rank * 4 / (d["ms_per_step"] * 4e-3), rel=1e-6)
    # every timed pass integrated a different shard (round 4); the counters are means over the passes' own tickets
    assert d["config"]["distinct_shards"] == 4 and d["roofline"]["rk4_steps_per_launch"] > 1000 * n_rank
    # --dump-outputs on N ranks: rank 0 writes the gathered results of the last timed pass, one column per sample
    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == ["status.npy", "summary.npy", "summary_nonfinite.npy"], files
    s, m, t = (np.load(tmp_path / "dump" / f) for f in files[1:] + files[:1])
    assert s.shape == m.shape == (_abi.SUMMARY_DIM, 2 * n_rank) and t.shape == (2 * n_rank,)
    assert all(x.dtype == np.float64 and np.isfinite(x).all() for x in (s, m, t))
    assert np.all(s[_abi.SUM_STEPS] > 0) and np.array_equal(t, np.round(t))


def test_bench_gpus_8_on_a_one_gpu_box_fails_clearly():
    """`python bench.py --gpus 8` typed as the driver types it, on a box with fewer GPUs: a clear message and rc != 0
    from the launcher, which never initialises the GPU itself."""
    import torch
    if torch.cuda.device_count() >= 8:
        pytest.skip("this box really has 8 GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                            "ERPL_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], env=env, capture_output=True,
                       text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and f"8 GPUs requested, {torch.cuda.device_count()} visible" in r.stderr, r.stderr[-1500:]


def test_plain_bench_line_and_its_dumped_outputs(tmp_path):
    """A plain `bench.py` run (no --full) is the headline leg alone: the contract's keys and none of the blocks --full
    adds.  `--dump-outputs` writes the last timed pass's results; with the same arguments two runs dump the same bits -
    checked three batches deep (GPU_MAX_HW_QUEUES=4, the HIP default, which the package leaves alone when it is set) as
    well as at the package's own depth - and with --shards 1 (every pass replays shard 0) the dumped status words give
    the line's own end reasons."""
    import json
    n = 16384
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--samples-per-gpu", str(n)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    got = {}
    for name, extra, queues in (("a", [], "4"), ("b", [], "4"), ("c", [], "24"), ("replay", ["--shards", "1"], "24")):
        r = subprocess.run(base + extra + ["--dump-outputs", str(tmp_path / name)], env=dict(env, GPU_MAX_HW_QUEUES=queues),
                           capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
            assert k in d, k
        for k in ("f32", "f64_gate", "parity", "apogee_match_rate", "cpu_baseline", "cfg5_share", "api_end_to_end"):
            assert k not in d, k
        assert d["steps"] == 2 and d["dtype"] == "f64_fast" and d["unit"] == "trajectories/s"
        assert d["config"]["passes_in_flight"] == (3 if queues == "4" else 8)
        assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3), rel=1e-6)
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["status.npy", "summary.npy", "summary_nonfinite.npy"], files
        for f in files:
            x = np.load(tmp_path / name / f)
            assert x.dtype == np.float64 and np.isfinite(x).all(), f
        s, t = np.load(tmp_path / name / "summary.npy"), np.load(tmp_path / name / "status.npy")
        marks = np.load(tmp_path / name / "summary_nonfinite.npy")
        s = np.select([marks == 1, marks == 2, marks == 3], [np.nan, np.inf, -np.inf], s)
        assert s.shape == (_abi.SUMMARY_DIM, n) and t.shape == (n,)
        assert np.array_equal(t, np.round(t)) and np.all(s[_abi.SUM_STEPS] > 0)
        got[name] = d, s, t
    (_, sa, ta), (_, sb, tb), (_, sc, tc) = got["a"], got["b"], got["c"]
    assert np.array_equal(sa, sb, equal_nan=True) and np.array_equal(ta, tb)
    assert np.array_equal(sa, sc, equal_nan=True) and np.array_equal(ta, tc)
    d, _, t = got["replay"]
    st = t.astype(np.int64)
    assert d["end_reasons"] == {k: int(np.sum((st & 0xFF) == v)) for k, v in
                                (("max_time", 0), ("ground", 1), ("altitude_100km", 2), ("coast", 3), ("apogee", 4))}


def test_bench_line_with_one_replayed_shard_and_with_a_shard_per_pass():
    """`bench.py` on one GPU at a small size: the default integrates a different resident shard in every timed pass,
    `--shards 1` replays one (the method of rounds 1-3); either way ONE JSON line with the contract's keys, the roofline of
    the dominant kernel from the timed passes' own device counters, and the parity block of the first timed pass (shard 0),
    which both methods run on the same samples: the same match report."""
    import json
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--samples-per-gpu", "16384",
            "--full", "--cpu-seconds", "1", "--no-cfg5", "--no-api"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    got = {}
    for name, extra in (("per_pass", []), ("replay", ["--shards", "1"])):
        r = subprocess.run(base + extra, env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = got[name] = json.loads(lines[0])
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config", "roofline", "cpu_baseline", "parity"):
            assert k in d, k
        assert d["config"]["distinct_shards"] == (3 if name == "per_pass" else 1)
        assert d["roofline"]["frac"] == pytest.approx(d["roofline"]["achieved"] / d["roofline"]["peak"])
        assert d["parity"]["timed_shard_vs_fp64_gate_kernel"]["n"] == 16384
        assert d["parity"]["timed_shard_vs_fp64_gate_kernel"]["same_end_reason"] == 1.0
    a, b = (got[k]["parity"]["timed_shard_vs_fp64_gate_kernel"] for k in ("per_pass", "replay"))
    assert a == b                                                   # shard 0 either way
    assert "other_timed_shards_vs_fp64_gate_kernel" in got["per_pass"]["parity"]
    assert "other_timed_shards_vs_fp64_gate_kernel" not in got["replay"]["parity"]
