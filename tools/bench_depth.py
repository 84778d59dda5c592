#!/usr/bin/env python3
"""erpl_mc_corridor_depth on the capture of a real f64_fast run and on synthetic rows, beside erpl_mc_corridor_bands on the
same matrix in the same process, and against the NumPy restatement in one host process.

Every GPU step runs in a child process of its own under its own time limit (`--limit` seconds); the first step that fails
or runs out of time ends the run.  Warm (`--warmup` calls), median of `--calls` host-timed calls, every window closed by a
device synchronise:

  capture     (3, 256, `--n`): `--n` planar liquid trajectories captured at `--stride` and resampled onto the default grid
              (the matrix of section 8.7), under the outlier filter's reason bytes
  synth M     (3, 256, M) for every `--m`: synthetic normal rows with 2 % NaN and 10 % masked columns (section 8.7's)
  paths M     (3, 256, M) for every `--paths` (<= the built-in LDS limit): the LDS path against the global path on the same
              data through lds_limit
Per step: the whole call; the kernels of one call by name from the profiler's kernel records where it gives any - the rank
pass alone is the unit's rank kernels plus, on the global path, the sort kernels beyond those of the LDS-path call (the
selection's sorts are in both) - else UNMEASURED; erpl_mc_corridor_bands on the same matrix; and the restatement (np.sort +
np.searchsorted per row, the two terms) on `--host-rows` rows, EXTRAPOLATED linearly to all rows.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXAMPLE_IC = {"position": [0.0, 0.0, 10.0], "velocity": [0, 0, 0.0], "attitude": [0.0, -1.5507963267948966, 0.0],
              "angular_velocity": [0.0, 0.0, 0.0]}
Q = (0.05, 0.25, 0.5, 0.75, 0.95)
RANK_KERNELS = ("erpl_depth_rank_lds", "erpl_depth_keys", "erpl_depth_offsets", "erpl_depth_lookup")


def wall(fn, warmup, calls):
    import torch
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


def kernels_of(fn):
    """Device time of one call by kind of kernel, in ms, from the profiler; None where it records no kernel."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {"rank_kernels": 0.0, "sort_kernels": 0.0, "other_depth_kernels": 0.0}
        seen = 0
        for ev in prof.events():
            us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
            if us <= 0.0:
                continue
            name = ev.name
            if any(k in name for k in RANK_KERNELS):
                out["rank_kernels"] += 1e-3 * us
            elif "erpl_depth_" in name:
                out["other_depth_kernels"] += 1e-3 * us
            elif "rocprim" in name or "radix" in name or "sort" in name:
                out["sort_kernels"] += 1e-3 * us
            else:
                continue
            seen += 1
        return out if seen else None
    except Exception as e:   # a profiler that cannot run here is not the benchmark's failure
        return {"error": repr(e)}


def host_rows(rows, keep):
    """The restatement's work on some rows: ranks, pair counts, the two terms."""
    t0 = time.perf_counter()
    for row in rows:
        p = keep & np.isfinite(row)
        xs = row[p]
        n = np.int64(len(xs))
        if n < 2:
            continue
        s = np.sort(xs)
        a = np.searchsorted(s, xs, side="left").astype(np.int64)
        b = n - np.searchsorted(s, xs, side="right").astype(np.int64)
        c2 = n * (n - 1) // 2
        (c2 - a * (a - 1) // 2 - b * (b - 1) // 2).astype(np.float64) / np.float64(c2), (n - a).astype(np.float64) / np.float64(n)
    return time.perf_counter() - t0


def measure(eng, values, mask, args, limits):
    """The whole call per lds_limit in `limits` (name -> value), the bands beside it, the restatement on some rows."""
    C, T, m = (int(s) for s in values.shape)
    res = {"shape": [C, T, m], "matrix_bytes": C * T * m * 8}
    for name, limit in limits.items():
        fn = lambda: eng.corridor_depth(values, mask=mask, lds_limit=limit)   # noqa: E731
        w = wall(fn, args.warmup, args.calls)
        k = kernels_of(fn)
        w["kernels_ms"] = k if k is not None else "UNMEASURED"
        res[name] = w
    if "lds" in res and "global" in res and isinstance(res["lds"]["kernels_ms"], dict) and "rank_kernels" in res["lds"]["kernels_ms"] \
            and isinstance(res["global"]["kernels_ms"], dict) and "rank_kernels" in res["global"]["kernels_ms"]:
        a, b = res["lds"]["kernels_ms"], res["global"]["kernels_ms"]
        res["rank_pass_ms"] = {"lds": a["rank_kernels"], "global": b["rank_kernels"] + b["sort_kernels"] - a["sort_kernels"]}
    else:
        only = next(iter(limits))
        k = res[only]["kernels_ms"]
        res["rank_pass_ms"] = {only: k["rank_kernels"] + (k["sort_kernels"] if only == "global" else 0.0),
                               "note": "global: with the selection's sorts"} if isinstance(k, dict) and "rank_kernels" in k else "UNMEASURED"
    res["bands"] = wall(lambda: eng.corridor_bands(values, mask, quantiles=Q), args.warmup, args.calls)
    rows = values.reshape(-1, m)[:: max(1, C * T // args.host_rows)][:args.host_rows].cpu().numpy()
    keep = np.ones(m, dtype=bool) if mask is None else (mask == 0).cpu().numpy()
    sec = host_rows(rows, keep)
    res["numpy"] = {"rows_timed": len(rows), "rows_s": sec, "rows_s_EXTRAPOLATED": sec * C * T / len(rows)}
    return res


def synthetic(eng, m):
    import torch
    gen = torch.Generator(device=eng.device).manual_seed(7)
    x = torch.randn((3, 256, m), dtype=torch.float64, device=eng.device, generator=gen)
    x[torch.rand((3, 256, m), device=eng.device, generator=gen) < 0.02] = float("nan")
    mask = (torch.rand((m,), device=eng.device, generator=gen) < 0.1).to(torch.uint8)
    return x, mask


def step(args):
    import torch  # noqa: F401
    from erpl_monte_carlo_sim_amd import _abi, analysis, models, sampling
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    eng = shared_engine(None)
    kind, _, size = args.step.partition(":")
    if kind == "capture":
        mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
        eng.set_config(mc._config())
        cap = int(np.ceil(mc.max_time / min(mc.dt_initial, 0.005) / args.stride)) + 4
        db = sampling.synthetic_dispersions(args.n, mc.rocket, mc.motor, mc.wind_model, dict(EXAMPLE_IC), eng.device,
                                            precision=_abi.PREC_F64_FAST, seed=1234, uncertainty=mc.uncertainty_params,
                                            base_altitude_profile=mc.base_altitude_profile, base_wind_profile=mc.base_wind_profile,
                                            planar=True, engine=eng)
        summ, status, traj, tlen = eng.run(db, traj_ids=np.arange(args.n), traj_stride=args.stride, traj_cap=cap)
        eng.synchronize()
        values = eng.corridor_resample(traj, tlen)
        _, ana, why = analysis._filter(summ, status, eng)
        del traj
        limits = {"lds": 0, "global": 1} if args.n <= _abi.DEPTH_LDS_MAX else {"global": 0}
        res = measure(eng, values, why, args, limits)
        res["n_valid"] = int(ana.n_valid)
    else:
        m = int(size)
        x, mask = synthetic(eng, m)
        if kind == "paths":
            limits = {"lds": 0, "global": 1}
        else:
            limits = {"lds": 0} if m <= _abi.DEPTH_LDS_MAX else {"global": 0}
        res = measure(eng, x, mask, args, limits)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--stride", type=int, default=25)
    ap.add_argument("--m", type=int, nargs="*", default=[131072, 1048576])
    ap.add_argument("--paths", type=int, nargs="*", default=[8192, 16384])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=12)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a step may take")
    ap.add_argument("--step", default=None, help="internal: the step a child process runs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["capture"] + [f"paths:{m}" for m in args.paths] + [f"synth:{m}" for m in args.m]
    res = {"n": args.n, "stride": args.stride, "warmup": args.warmup, "calls": args.calls}
    for s in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s] + \
              [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("n", "stride", "warmup", "calls", "host_rows")]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            res[s] = f"no result: over {args.limit} s"
            break
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            res[s] = f"no result: exit status {out.returncode}: {out.stderr[-400:]}"
            break
        res[s] = json.loads(line[-1][7:])
        print(f"# {s}: done", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
