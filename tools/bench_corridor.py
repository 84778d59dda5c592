#!/usr/bin/env python3
"""The trajectory corridor (erpl_mc_corridor_resample + erpl_mc_corridor_bands) on the capture of a real f64_fast run, and
the bands call alone on synthetic matrices, against NumPy in one host process.

Warm (`--warmup` calls), median of `--calls` host-timed calls, every window closed by a device synchronise:

  resample        `--n` planar liquid trajectories captured at `--stride` (the set of section 8.6) onto the default grid
                  (altitude, downrange, speed; 256 nodes 1 s apart); records/s and record bytes/s over the records WRITTEN
  resample, u=1   the same capture with record 1 made non-finite: the usable-prefix pass alone (it still streams every
                  record; every node but the first is NaN) - the figure to hold against section 8.6's pass 1
  envelope        erpl_mc_flight_envelope on the same capture, for the comparison on the same device and day
  bands           every row of that matrix under the outlier filter's reason bytes; then 3 x 256 rows of synthetic normal
                  values (2 % NaN) at each `--m`
  numpy           np.interp per trajectory and channel on `--host-traj` trajectories, np.quantile (five fractions) + mean +
                  std + min + max per row on `--host-rows` rows, one process, EXTRAPOLATED linearly to all of them
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from erpl_monte_carlo_sim_amd import _abi, analysis, models, sampling   # noqa: E402
from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer     # noqa: E402
from erpl_monte_carlo_sim_amd.simulator import shared_engine            # noqa: E402

EXAMPLE_IC = {"position": [0.0, 0.0, 10.0], "velocity": [0, 0, 0.0], "attitude": [0.0, -1.5507963267948966, 0.0],
              "angular_velocity": [0.0, 0.0, 0.0]}
HBM = 8.0e12
Q = (0.05, 0.25, 0.5, 0.75, 0.95)


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


def rate(w, records):
    s = w["median_ms"] * 1e-3
    w.update({"records_per_s": records / s, "record_bytes_per_s": records * 120 / s, "share_of_hbm": records * 120 / s / HBM})
    return w


def host_rows(rows, keep):
    t0 = time.perf_counter()
    for row in rows:
        v = row[keep & np.isfinite(row)]
        if len(v):
            np.quantile(v, Q), v.mean(), v.std(), v.min(), v.max()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--stride", type=int, default=25)
    ap.add_argument("--m", type=int, nargs="*", default=[131072, 1048576])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-traj", type=int, default=256)
    ap.add_argument("--host-rows", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    eng = shared_engine(None)
    eng.set_config(mc._config())
    cap = int(np.ceil(mc.max_time / min(mc.dt_initial, 0.005) / args.stride)) + 4
    db = sampling.synthetic_dispersions(args.n, mc.rocket, mc.motor, mc.wind_model, dict(EXAMPLE_IC), eng.device,
                                        precision=_abi.PREC_F64_FAST, seed=1234, uncertainty=mc.uncertainty_params,
                                        base_altitude_profile=mc.base_altitude_profile, base_wind_profile=mc.base_wind_profile,
                                        planar=True, engine=eng)
    summ, status, traj, tlen = eng.run(db, traj_ids=np.arange(args.n), traj_stride=args.stride, traj_cap=cap)
    ids = eng._keep
    eng.synchronize()
    records = int(tlen.clamp(0, cap).sum())
    res = {"n": args.n, "stride": args.stride, "cap": cap, "records": records, "record_bytes": records * 120}
    spec = eng.corridor_spec()
    shape = (spec.n_channels, spec.n_nodes, args.n)
    values = torch.full(shape, float("nan"), dtype=torch.float64, device=eng.device)
    res["resample"] = rate(wall(lambda: eng.corridor_resample(traj, tlen, out=values), args.warmup, args.calls), records)
    res["resample_hold"] = rate(wall(lambda: eng.corridor_resample(traj, tlen, hold=True, out=values), args.warmup, args.calls), records)
    res["envelope"] = rate(wall(lambda: eng.flight_envelope(db, ids, traj, tlen), args.warmup, args.calls), records)
    eng.corridor_resample(traj, tlen, out=values)
    _, ana, why = analysis._filter(summ, status, eng)
    res["n_valid"] = int(ana.n_valid)
    res["bands"] = wall(lambda: eng.corridor_bands(values, why, quantiles=Q), args.warmup, args.calls)
    res["bands"]["rows"] = shape[0] * shape[1]

    # the host: np.interp on some trajectories, the row statistics on some rows
    host_traj = min(args.host_traj, args.n)
    rec, lens = traj[:host_traj].cpu().numpy(), tlen[:host_traj].cpu().numpy()
    nodes = spec.t0 + np.arange(spec.n_nodes) * spec.dt
    t0 = time.perf_counter()
    for j in range(host_traj):
        r = rec[j, :lens[j]]
        ts = r[:, 0] - r[0, 0]
        for ch in (r[:, 3], np.sqrt(r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]),
                   np.sqrt((r[:, 4] * r[:, 4] + r[:, 5] * r[:, 5]) + r[:, 6] * r[:, 6])):
            np.interp(nodes, ts, ch, left=np.nan, right=np.nan)
    sec = time.perf_counter() - t0
    host_vals, keep = values.cpu().numpy().reshape(-1, args.n), (why == 0).cpu().numpy()
    pick = np.linspace(0, host_vals.shape[0] - 1, args.host_rows).astype(int)
    sec_rows = host_rows(host_vals[pick], keep)
    res["numpy"] = {"interp_trajectories_timed": host_traj, "interp_s": sec, "interp_s_extrapolated": sec * args.n / host_traj,
                    "rows_timed": len(pick), "rows_s": sec_rows,
                    "rows_s_extrapolated": sec_rows * host_vals.shape[0] / len(pick)}

    # the usable-prefix pass alone
    traj[:, 1, 3] = float("nan")
    res["resample_u1"] = rate(wall(lambda: eng.corridor_resample(traj, tlen, out=values), args.warmup, args.calls), records)
    res["envelope_u1"] = rate(wall(lambda: eng.flight_envelope(db, ids, traj, tlen), args.warmup, args.calls), records)
    del traj, values, db
    torch.cuda.empty_cache()

    # the bands call alone
    res["bands_alone"] = []
    for m in args.m:
        gen = torch.Generator(device=eng.device).manual_seed(7)
        x = torch.randn((3, 256, m), dtype=torch.float64, device=eng.device, generator=gen)
        x[torch.rand((3, 256, m), device=eng.device, generator=gen) < 0.02] = float("nan")
        mask = (torch.rand((m,), device=eng.device, generator=gen) < 0.1).to(torch.uint8)
        w = wall(lambda: eng.corridor_bands(x, mask, quantiles=Q), args.warmup, args.calls)
        xs = x.reshape(-1, m)[:: max(1, 768 // args.host_rows)][:args.host_rows].cpu().numpy()
        sec_rows = host_rows(xs, (mask == 0).cpu().numpy())
        w.update({"m": m, "rows": 768, "matrix_bytes": 768 * m * 8, "matrix_bytes_per_s_10_reads": 10 * 768 * m * 8 / (w["median_ms"] * 1e-3),
                  "numpy_rows_timed": len(xs), "numpy_rows_s": sec_rows, "numpy_rows_s_extrapolated": sec_rows * 768 / len(xs)})
        res["bands_alone"].append(w)
        del x, mask
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
