#!/usr/bin/env python3
"""erpl_mc_qmc (TrajectoryEngine.qmc) at the primitive tensor of a K = 100 run (319 rows on the dimensions of
sampling.qmc_dims: 315 normal and 2 uniform Sobol' rows, 2 pad rows) and `--columns` columns (default 1 048 576, one
DEVICE_CHUNK of run_monte_carlo_device), and what the design buys on flown outputs.  Recorded, not asserted.

  native            HIP-event time of the call on its stream, warm, the output tensor allocated before: median of `--calls`
                    after `--warmup` warm-up calls.  Beside the full call its parts, each by leaving one out: RAW (no
                    scramble, no jitter), every row uniform (no PPND16), every row a pad row (no Sobol' work at all: the
                    jitter and PPND16 alone), and erpl_mc_design LHS of the same shape in the same process
  written bytes     8 bytes per value, the only memory traffic of the kernel beside 128 bytes of direction numbers per
                    workgroup, over that time, beside the HBM copy rate of MI355X_MICROARCH.md (6.29 TB/s measured)
  SobolEngine       torch.quasirandom.SobolEngine(319, scramble=True).draw(columns, dtype=float64) - a host generator: the
                    time is wall clock (median of 3), the upload and the normal quantile are not in it; the same shape
                    unless `--torch-columns` asks for fewer columns, which are then scaled
  payoff            planar flights, `--flights` per run, `--seeds` seeds: the standard deviation over the seeds of the mean
                    first-apogee altitude and of P(range > c) among the regular flights (a finite range of at most
                    `--max-range`: the freak mode beyond it is left out, as in bench_subset.py), c the 0.95 quantile of the
                    range of the regular flights of all 'random' runs pooled
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

from erpl_monte_carlo_sim_amd import _abi, models, sampling      # noqa: E402
from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer   # noqa: E402
from erpl_monte_carlo_sim_amd.simulator import shared_engine          # noqa: E402

K = 100
HBM_TBS = {"measured_copy": 6.29, "spec": 8.0}
EXAMPLE_IC = {"position": [0.0, 0.0, 10.0], "velocity": [0, 0, 0.0], "attitude": [0.0, -np.pi / 2 + 0.02, 0.0],
              "angular_velocity": [0.0, 0.0, 0.0]}


def event_ms(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=1 << 20)
    ap.add_argument("--torch-columns", type=int, default=0, help="0: the columns of the native call")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--flights", type=int, default=1024)
    ap.add_argument("--max-range", type=float, default=20000.0)
    ap.add_argument("--out", default="profiles/qmc_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = shared_engine(dev)
    rows, n = sampling.primitive_rows(K), args.columns
    kinds = [_abi.DESIGN_NORMAL] * (rows - 2) + [_abi.DESIGN_UNIFORM] * 2
    uniform = [_abi.DESIGN_UNIFORM] * rows
    dims = sampling.qmc_dims(K)
    out = torch.empty((rows, n), dtype=torch.float64, device=dev)
    nbytes = 8 * rows * n
    gen = {"columns": n, "rows": rows, "sobol_rows": sum(d >= 0 for d in dims), "written_bytes": nbytes}
    cases = (("erpl_mc_qmc_owen", lambda: eng.qmc(kinds, n, 1234, dims=dims, out=out)),
             ("erpl_mc_qmc_owen_block_4096", lambda: eng.qmc(kinds, n, 1234, dims=dims, block=4096, out=out)),
             ("erpl_mc_qmc_owen_all_uniform", lambda: eng.qmc(uniform, n, 1234, dims=dims, out=out)),
             ("erpl_mc_qmc_raw", lambda: eng.qmc(kinds, n, 1234, dims=dims, scramble="raw", out=out)),
             ("erpl_mc_qmc_raw_all_uniform", lambda: eng.qmc(uniform, n, 1234, dims=dims, scramble="raw", out=out)),
             ("erpl_mc_qmc_all_pad_random", lambda: eng.qmc(kinds, n, 1234, dims=[-1] * rows, out=out)),
             ("erpl_mc_design_lhs", lambda: eng.design(kinds, n, 1234, kind="lhs", out=out)),
             ("erpl_mc_design_random", lambda: eng.design(kinds, n, 1234, kind="random", out=out)))
    for name, fn in cases:
        t = event_ms(fn, args.warmup, args.calls)
        t["written_TB_per_s"] = nbytes / (1e-3 * t["median_ms"]) / 1e12
        t["share_of_measured_hbm_copy_rate"] = t["written_TB_per_s"] / HBM_TBS["measured_copy"]
        gen[name] = t
        print(name, json.dumps(t), flush=True)
    eng.synchronize()
    del out
    torch.cuda.empty_cache()
    walls, tcols = [], args.torch_columns or n
    for _ in range(3):
        t0 = time.perf_counter()
        drawn = torch.quasirandom.SobolEngine(rows, scramble=True, seed=1234).draw(tcols, dtype=torch.float64)
        walls.append(1e3 * (time.perf_counter() - t0))
        del drawn
    gen["torch_sobol_engine"] = {"columns": tcols, "wall_ms": statistics.median(walls), "walls_ms": walls,
                                 "scaled_to_columns_ms": statistics.median(walls) * n / tcols,
                                 "note": "host generator (table, scramble and draw), uniforms only, no upload, no normal quantile"}
    gen["qmc_over_design_lhs"] = gen["erpl_mc_qmc_owen"]["median_ms"] / gen["erpl_mc_design_lhs"]["median_ms"]
    print(json.dumps(gen["torch_sobol_engine"]), flush=True)
    report = {"what": "HIP-event milliseconds per call, warm, median; written bytes = 8 * rows * columns; the payoff: standard "
                      "deviation over seeds of two estimates from planar runs",
              "guide_hbm_TB_per_s": HBM_TBS, "generation": gen}

    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    apogee, ranges = {}, {}
    for design in ("random", "lhs", "qmc"):
        apogee[design], ranges[design] = [], []
        for seed in range(args.seeds):
            run = mc.run_monte_carlo_device(dict(EXAMPLE_IC), args.flights, seed=seed, planar=True, design=design)
            x = run["summary"][_abi.SUM_FIRST_APOGEE_ALT]
            apogee[design].append(float(x[torch.isfinite(x)].mean()))
            ranges[design].append(run["summary"][_abi.SUM_RANGE].cpu().numpy())
    regular = {d: [r[np.isfinite(r) & (r <= args.max_range)] for r in v] for d, v in ranges.items()}
    c = float(np.quantile(np.concatenate(regular["random"]), 0.95))
    tail = {d: [float(np.mean(r > c)) for r in v] for d, v in regular.items()}
    sd_mean = {d: float(np.std(v, ddof=1)) for d, v in apogee.items()}
    sd_tail = {d: float(np.std(v, ddof=1)) for d, v in tail.items()}
    report["payoff"] = {"flights": args.flights, "seeds": args.seeds, "planar": True,
                        "mean_first_apogee_altitude": {"means": apogee, "std_of_mean": sd_mean,
                                                       "std_ratio_qmc_over_lhs": sd_mean["qmc"] / sd_mean["lhs"],
                                                       "std_ratio_qmc_over_random": sd_mean["qmc"] / sd_mean["random"]},
                        "p_range_above_q95": {"threshold_m": c, "max_range_m": args.max_range,
                                              "regular_flights_mean": {d: float(np.mean([len(r) for r in v])) for d, v in regular.items()},
                                              "estimates": tail, "std_of_estimate": sd_tail,
                                              "binomial_std_iid": float(np.sqrt(0.05 * 0.95 / args.flights)),
                                              "std_ratio_qmc_over_lhs": sd_tail["qmc"] / sd_tail["lhs"],
                                              "std_ratio_qmc_over_random": sd_tail["qmc"] / sd_tail["random"]}}
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("means", "estimates")} if isinstance(v, dict) else v
                      for k, v in report["payoff"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
