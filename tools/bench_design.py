#!/usr/bin/env python3
"""erpl_mc_design (TrajectoryEngine.design) against the draws it replaces, at the primitive tensor of a K = 100 run
(17 + 3 K + 2 = 319 rows: 317 normal rows, 2 uniform rows) and `--columns` columns (default 1 048 576, one DEVICE_CHUNK of
run_monte_carlo_device), and what a stratified design buys on a flown output.  Recorded, not asserted.

  native            HIP-event time of the call on its stream, warm, the output tensor allocated before: median of `--calls`
                    after `--warmup` warm-up calls; LHS, RANDOM and LHS with all rows uniform (no normal quantile)
  written bytes     8 bytes per value, the only memory traffic of the kernel, over that time, beside the HBM copy rate of
                    MI355X_MICROARCH.md (6.29 TB/s measured, 8.0 TB/s spec)
  primitive_draws   sampling.primitive_draws (torch.randn + torch.rand + cat), the i.i.d. draws of today's designs
  torch LHS         the textbook form in torch: argsort of random keys per row, (rank + rand) / n, torch.special.ndtri on
                    the normal rows - needs the whole row resident and cannot be cut into windows
  variance          standard deviation over `--seeds` seeds of the mean first-apogee altitude of
                    run_monte_carlo_device(n = `--flights`, planar), design 'lhs' against 'random'
"""
import argparse
import json
import os
import statistics
import sys

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


def torch_lhs(n, rows_normal, rows_uniform, device, seed):
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    rows = rows_normal + rows_uniform
    rank = torch.argsort(torch.rand((rows, n), generator=gen, dtype=torch.float64, device=device), dim=1)
    p = (rank.to(torch.float64) + torch.rand((rows, n), generator=gen, dtype=torch.float64, device=device)) / n
    p[:rows_normal] = torch.special.ndtri(p[:rows_normal])
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, nargs="+", default=[1 << 20])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--flights", type=int, default=1024)
    ap.add_argument("--out", default="profiles/design_native_vs_torch.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = shared_engine(dev)
    rows = sampling.primitive_rows(K)
    kinds = [_abi.DESIGN_NORMAL] * (rows - 2) + [_abi.DESIGN_UNIFORM] * 2
    report = {"what": "HIP-event milliseconds per call, warm; written bytes = 8 * rows * columns; the variance study: standard "
                      "deviation over seeds of the mean first-apogee altitude of a planar run",
              "guide_hbm_TB_per_s": HBM_TBS, "rows": rows, "sizes": []}
    for n in args.columns:
        out = torch.empty((rows, n), dtype=torch.float64, device=dev)
        nbytes = 8 * rows * n
        row = {"columns": n, "written_bytes": nbytes}
        for name, kind, kk in (("lhs", "lhs", kinds), ("random", "random", kinds), ("lhs_centred", "lhs_centred", kinds),
                               ("lhs_all_uniform", "lhs", [_abi.DESIGN_UNIFORM] * rows),
                               ("lhs_block_4096", "lhs", kinds)):
            block = 4096 if name == "lhs_block_4096" else 0
            t = event_ms(lambda: eng.design(kk, n, 1234, kind=kind, block=block, out=out), args.warmup, args.calls)
            t["written_TB_per_s"] = nbytes / (1e-3 * t["median_ms"]) / 1e12
            t["share_of_measured_hbm_copy_rate"] = t["written_TB_per_s"] / HBM_TBS["measured_copy"]
            row["erpl_mc_design_" + name] = t
        eng.synchronize()
        del out
        row["primitive_draws"] = event_ms(lambda: sampling.primitive_draws(n, K, dev, 1234), args.warmup, args.calls)
        row["torch_argsort_lhs"] = event_ms(lambda: torch_lhs(n, rows - 2, 2, dev, 1234), 1, max(3, args.calls // 3))
        for name in ("primitive_draws", "torch_argsort_lhs"):
            row[name + "_over_native_lhs"] = row[name]["median_ms"] / row["erpl_mc_design_lhs"]["median_ms"]
        report["sizes"].append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    means = {}
    for design in ("random", "lhs"):
        means[design] = []
        for seed in range(args.seeds):
            run = mc.run_monte_carlo_device(dict(EXAMPLE_IC), args.flights, seed=seed, planar=True, design=design)
            x = run["summary"][_abi.SUM_FIRST_APOGEE_ALT]
            means[design].append(float(x[torch.isfinite(x)].mean()))
    sd = {d: float(np.std(v, ddof=1)) for d, v in means.items()}
    report["variance"] = {"flights": args.flights, "seeds": args.seeds, "planar": True, "row": "first_apogee_altitude",
                          "means": means, "std_of_mean": sd, "std_ratio_lhs_over_random": sd["lhs"] / sd["random"],
                          "variance_ratio_lhs_over_random": (sd["lhs"] / sd["random"]) ** 2}
    print(json.dumps(report["variance"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
