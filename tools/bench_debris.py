#!/usr/bin/env python3
"""The debris footprint (erpl_mc_debris) on the capture of tools/bench_iip.py, beside erpl_mc_impact_points on the same
capture in the same process and beside the NumPy restatement tests/debris_ref.py.

Warm (`--warmup` calls), median of `--calls` host-timed calls, every window closed by a device synchronise:

  capture        `--n` planar liquid trajectories captured at `--stride`
  debris         `--nodes` nodes spread over max_time x `--fragments` fragments with beta log-spaced from `--beta-min` to
                 `--beta-max` and one of +inf, dv = `--dv`, dt = `--dt`: the time of the call, with and without its summary
  steps          the trace holds fall times, not step counts: a landed job took AT LEAST ceil(TFALL / dt) RK4 steps, and
                 exactly that many where no step was halved.  RK4 steps and RHS evaluations per second are this LOWER BOUND
                 over the call's time; the restated jobs below give the true count on a few jobs for comparison
  utilisation    as DESIGN.md 8.11 defines it: sum(steps over lanes) / (64 * sum over waves of the wave's longest fall), a
                 wave being 64 neighbouring trajectories at one (node, fragment)
  impact_points  erpl_mc_impact_points on the same capture, same nodes, same dt
  numpy          tests/debris_ref.py on the longest fall of `--host-jobs` trajectories, one process, EXTRAPOLATED by RK4
                 steps (lower bound, as above) to all landed jobs

`--lib PATH` loads another build of the library (an experiment build, never the product): how the dispatch orders and the
register caps of DESIGN.md 8.18 were compared.
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
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine             # noqa: E402
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
    """steps [rows, n]: busy lane-steps over 64 x the longest fall of every wave of 64 neighbouring trajectories of a row."""
    rows, m = steps.shape
    a = np.pad(steps, ((0, 0), (0, (-m) % 64)))
    return float(steps.sum()) / (64.0 * float(a.reshape(rows, -1, 64).max(axis=2).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--stride", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=16)
    ap.add_argument("--fragments", type=int, default=8)
    ap.add_argument("--beta-min", type=float, default=5.0)
    ap.add_argument("--beta-max", type=float, default=5000.0)
    ap.add_argument("--dv", type=float, default=30.0)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--max-steps", type=int, default=200000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-jobs", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    eng = TrajectoryEngine(torch.device("cuda", 0), lib_path=args.lib)
    cfg = mc._config()
    eng.set_config(cfg)
    cap = int(np.ceil(mc.max_time / min(mc.dt_initial, 0.005) / args.stride)) + 4
    rs = max(1, (cap - 4) // args.nodes)
    F = args.fragments
    betas = [float(b) for b in np.geomspace(args.beta_min, args.beta_max, F - 1)] + [float("inf")] if F > 1 else [args.beta_min]
    frags = [(b, 0.0 if np.isinf(b) else args.dv) for b in betas]
    db = sampling.synthetic_dispersions(args.n, mc.rocket, mc.motor, mc.wind_model, dict(EXAMPLE_IC), eng.device,
                                        precision=_abi.PREC_F64_FAST, seed=1234, uncertainty=mc.uncertainty_params,
                                        base_altitude_profile=mc.base_altitude_profile, base_wind_profile=mc.base_wind_profile,
                                        planar=True, engine=eng)
    res = {"label": args.label, "n": args.n, "stride": args.stride, "cap": cap, "nodes": args.nodes, "record_stride": rs,
           "fragments": [["inf" if np.isinf(b) else b, dv] for b, dv in frags], "dt": args.dt, "max_steps": args.max_steps}
    box = {}

    def capture():
        box["run"] = eng.run(db, traj_ids=np.arange(args.n), traj_stride=args.stride, traj_cap=cap)
        eng.synchronize()

    res["capture"] = wall(capture, 1, 3)
    summ, status, traj, tlen = box["run"]
    ids = eng._keep
    values = torch.full((_abi.IIP_CH_COUNT, args.nodes * F, args.n), float("nan"), dtype=torch.float64, device=eng.device)
    call = lambda **kw: eng.debris(db, ids, traj, tlen, frags, nodes=args.nodes, record_stride=rs, dt=args.dt,
                                   max_steps=args.max_steps, seed=1, out=values, **kw)
    w = wall(call, args.warmup, args.calls)
    res["debris_no_summary"] = wall(lambda: call(summary=False), 0, args.calls)
    _, deb = call()
    torch.cuda.synchronize()
    v, s = values.cpu().numpy(), deb.cpu().numpy()
    tfall = v[_abi.IIP_CH_TFALL]
    landed = np.isfinite(tfall)
    steps = np.where(landed, np.ceil(np.nan_to_num(tfall) / args.dt), 0.0)
    evaluated = (np.arange(args.nodes * F)[:, None] // F) < s[_abi.DEBRIS_NODES][None, :]
    sec = w["median_ms"] * 1e-3
    per_fragment = steps.reshape(args.nodes, F, args.n).sum(axis=(0, 2))
    w.update({"jobs": args.nodes * F * args.n, "evaluated_jobs": int(evaluated.sum()), "landed_jobs": int(landed.sum()),
              "rk4_steps_lower_bound": float(steps.sum()), "longest_fall_steps_lower_bound": float(steps.max()),
              "rk4_steps_lower_bound_per_fragment": [float(x) for x in per_fragment],
              "jobs_per_s": float(evaluated.sum()) / sec, "rk4_steps_per_s_lower_bound": float(steps.sum()) / sec,
              "rhs_evaluations_per_s_lower_bound": 4.0 * float(steps.sum()) / sec})
    res["debris"] = w
    res["lane_utilisation"] = utilisation(steps)

    # the intact vehicle on the same capture, same nodes, same step
    iv = torch.full((_abi.IIP_CH_COUNT, args.nodes, args.n), float("nan"), dtype=torch.float64, device=eng.device)
    icall = lambda: eng.impact_points(db, ids, traj, tlen, nodes=args.nodes, record_stride=rs, dt=args.dt,
                                      max_steps=min(args.max_steps, _abi.IIP_MAX_STEPS), out=iv)
    g = wall(icall, args.warmup, args.calls)
    torch.cuda.synchronize()
    it = iv[_abi.IIP_CH_TFALL].cpu().numpy()
    isteps = np.where(np.isfinite(it), np.ceil(np.nan_to_num(it) / args.dt), 0.0)
    g.update({"rk4_steps": float(isteps.sum()), "rhs_evaluations_per_s": 4.0 * float(isteps.sum()) / (g["median_ms"] * 1e-3),
              "lane_utilisation": utilisation(isteps)})
    res["impact_points"] = g
    res["rhs_rate_over_impact_points"] = w["rhs_evaluations_per_s_lower_bound"] / g["rhs_evaluations_per_s"]

    # NumPy: the restatement on the longest fall of the first trajectories, extrapolated by steps
    if args.host_jobs > 0:
        import debris_ref
        from oracle import oracle as orc
        true_steps, bound_steps, t_host, done = 0.0, 0.0, 0.0, 0
        rec_host = traj[:args.host_jobs].cpu().numpy()
        for j in range(min(args.host_jobs, args.n)):
            hb1 = flatten.HostBatch(1, db.k_wind)
            hb1.rocket, hb1.motor = db.rocket[:, j:j + 1].cpu().numpy().copy(), db.motor[:, j:j + 1].cpu().numpy().copy()
            if db.k_wind:
                hb1.alt_grid, hb1.wind = db.alt_grid.cpu().numpy().copy(), db.wind[:, :, j:j + 1].cpu().numpy().copy()
            fall = debris_ref.Fall(orc, cfg, hb1, sid=j, dt=args.dt, max_steps=args.max_steps, seed=1)
            i = int(np.argmax(steps[:, j]))     # the trajectory's longest fall
            if not landed[i, j]:
                continue
            k, f = i // F, i % F
            t0 = time.perf_counter()
            got = fall.job(rec_host[j, k * rs], k, f, *frags[f])
            t_host += time.perf_counter() - t0
            true_steps += fall.steps
            bound_steps += steps[i, j]
            done += 1
            assert abs(got[_abi.IIP_CH_TFALL] - tfall[i, j]) <= 1e-9 * max(1.0, tfall[i, j]), (j, i, got, v[:, i, j])
        res["numpy"] = {"jobs_timed": done, "steps_timed": true_steps, "steps_timed_lower_bound": bound_steps, "seconds": t_host,
                        "seconds_extrapolated_by_steps": t_host / max(bound_steps, 1.0) * float(steps.sum())}
    line = json.dumps(res, allow_nan=False)   # strict JSON: beta = +inf is the string "inf"
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
