#!/usr/bin/env python3
"""The instantaneous impact points (erpl_mc_impact_points) on the capture of a real f64_fast run, against the gate flight
kernel's own RHS rate on the same device and against the NumPy restatement tests/iip_ref.py.

Warm (`--warmup` calls), median of `--calls` host-timed calls, every window closed by a device synchronise:

  capture         `--n` planar liquid trajectories captured at `--stride` (its cost goes next to the call's)
  impact_points   `--nodes` nodes spread over max_time, dt = `--dt`: the time of the call, nodes/s and RHS evaluations/s, the
                  latter as 4 * sum(ceil(TFALL / dt)) over the landed nodes of the trace itself (a node that does not land
                  counts max_steps steps if it was of physical size: an upper bound, reported apart)
  utilisation     on the host from the trace: sum(steps over lanes) / (64 * sum over waves of the wave's longest fall), for
                  both job orders - 64 neighbouring trajectories at one node, 64 neighbouring nodes of one trajectory
  gate flight     erpl_mc_run_batch of the same samples through the ERPL_PREC_F64 build without capture:
                  erpl_mc_last_stats steps * 4 over its time - the yardstick for RHS evaluations/s
  numpy           tests/iip_ref.py on `--host-nodes` landed nodes, one process, EXTRAPOLATED by RK4 steps to all of them

`--lib PATH` loads another build of the library (an experiment build, never the product).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from erpl_monte_carlo_sim_amd import _abi, flatten, models, sampling   # noqa: E402
from erpl_monte_carlo_sim_amd.engine import DeviceBatch, TrajectoryEngine   # noqa: E402
from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer     # noqa: E402

EXAMPLE_IC = {"position": [0.0, 0.0, 10.0], "velocity": [0, 0, 0.0], "attitude": [0.0, -1.5507963267948966, 0.0],
              "angular_velocity": [0.0, 0.0, 0.0]}


def wall(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


def utilisation(steps):
    """steps [nodes, n] -> (trajectory-fastest, node-fastest): busy lane-steps over 64 x the waves' longest falls."""
    nodes, n = steps.shape
    total = float(steps.sum())

    def waves(a):   # a [rows, lanes along the last axis]: groups of 64 along it
        rows, m = a.shape
        pad = (-m) % 64
        a = np.pad(a, ((0, 0), (0, pad)))
        return float(a.reshape(rows, -1, 64).max(axis=2).sum())

    return total / (64.0 * waves(steps)), total / (64.0 * waves(steps.T.copy()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--stride", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--max-steps", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-nodes", type=int, default=6)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="trajectory-fastest")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    eng = TrajectoryEngine(torch.device("cuda", 0), lib_path=args.lib)
    cfg = mc._config()
    eng.set_config(cfg)
    cap = int(np.ceil(mc.max_time / min(mc.dt_initial, 0.005) / args.stride)) + 4
    rs = max(1, (cap - 4) // args.nodes)
    db = sampling.synthetic_dispersions(args.n, mc.rocket, mc.motor, mc.wind_model, dict(EXAMPLE_IC), eng.device,
                                        precision=_abi.PREC_F64_FAST, seed=1234, uncertainty=mc.uncertainty_params,
                                        base_altitude_profile=mc.base_altitude_profile, base_wind_profile=mc.base_wind_profile,
                                        planar=True, engine=eng)
    res = {"label": args.label, "n": args.n, "stride": args.stride, "cap": cap, "nodes": args.nodes, "record_stride": rs,
           "dt": args.dt, "max_steps": args.max_steps}
    box = {}

    def capture():
        box["run"] = eng.run(db, traj_ids=np.arange(args.n), traj_stride=args.stride, traj_cap=cap)
        eng.synchronize()

    res["capture"] = wall(capture, 1, 3)
    summ, status, traj, tlen = box["run"]
    ids = eng._keep
    res["records"] = int(tlen.clamp(0, cap).sum())
    values = torch.full((_abi.IIP_CH_COUNT, args.nodes, args.n), float("nan"), dtype=torch.float64, device=eng.device)
    call = lambda **kw: eng.impact_points(db, ids, traj, tlen, nodes=args.nodes, record_stride=rs, dt=args.dt,
                                          max_steps=args.max_steps, out=values, **kw)
    w = wall(call, args.warmup, args.calls)
    res["impact_points_no_summary"] = wall(lambda: call(summary=False), 0, args.calls)
    _, iip = call()
    torch.cuda.synchronize()
    v, s = values.cpu().numpy(), iip.cpu().numpy()
    tfall = v[_abi.IIP_CH_TFALL]
    landed = np.isfinite(tfall)
    steps = np.where(landed, np.ceil(np.nan_to_num(tfall) / args.dt), 0.0)
    evaluated = np.arange(args.nodes)[:, None] < s[_abi.IIP_NODES][None, :]
    sec = w["median_ms"] * 1e-3
    w.update({"jobs": args.nodes * args.n, "evaluated_nodes": int(evaluated.sum()), "landed_nodes": int(landed.sum()),
              "rk4_steps_of_landed_nodes": float(steps.sum()), "longest_fall_steps": float(steps.max()),
              "nodes_per_s": float(evaluated.sum()) / sec, "rhs_evaluations_per_s": 4.0 * float(steps.sum()) / sec,
              "rhs_evaluations_upper_bound": 4.0 * float(steps.sum() + (evaluated & ~landed).sum() * args.max_steps)})
    res["impact_points"] = w
    u_traj, u_node = utilisation(steps)
    res["lane_utilisation"] = {"trajectory_fastest": u_traj, "node_fastest": u_node}

    # the gate flight kernel on the same samples: its RHS evaluations per second
    db64 = DeviceBatch(db.ic, db.rocket, db.motor, db.alt_grid, db.wind, _abi.PREC_F64)
    out64 = eng.alloc_outputs(args.n)
    g = wall(lambda: eng.run(db64, summary=out64[0], status=out64[1]), 1, 3)
    eng.synchronize()
    total_steps = float(eng.last_stats()[0])
    g.update({"rk4_steps": total_steps, "rhs_evaluations_per_s": 4.0 * total_steps / (g["median_ms"] * 1e-3)})
    res["gate_flight"] = g
    res["rhs_rate_over_gate_flight"] = w["rhs_evaluations_per_s"] / g["rhs_evaluations_per_s"]

    # NumPy: the restatement on a few landed nodes of the first trajectories, extrapolated by steps
    if args.host_nodes > 0:
        import iip_ref
        from oracle import oracle as orc
        timed_steps, t_host, done = 0.0, 0.0, 0
        rec_host, len_host = traj[:args.host_nodes].cpu().numpy(), tlen[:args.host_nodes].cpu().numpy()
        for j in range(min(args.host_nodes, args.n)):
            hb1 = flatten.HostBatch(1, db.k_wind)
            hb1.rocket, hb1.motor = db.rocket[:, j:j + 1].cpu().numpy().copy(), db.motor[:, j:j + 1].cpu().numpy().copy()
            if db.k_wind:
                hb1.alt_grid, hb1.wind = db.alt_grid.cpu().numpy().copy(), db.wind[:, :, j:j + 1].cpu().numpy().copy()
            fall = iip_ref.Fall(orc, cfg, hb1, dt=args.dt, max_steps=args.max_steps)
            k = int(np.argmax(steps[:, j]))     # the trajectory's longest fall
            if not landed[k, j]:
                continue
            t0 = time.perf_counter()
            got = fall.node(rec_host[j, k * rs])
            t_host += time.perf_counter() - t0
            timed_steps += fall.steps
            done += 1
            assert abs(got[_abi.IIP_CH_TFALL] - tfall[k, j]) <= 1e-9 * max(1.0, tfall[k, j]), (j, k, got, v[:, k, j])
        res["numpy"] = {"nodes_timed": done, "steps_timed": timed_steps, "seconds": t_host,
                        "seconds_extrapolated_by_steps": t_host / max(timed_steps, 1.0) * float(steps.sum())}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
