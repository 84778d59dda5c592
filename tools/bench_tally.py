#!/usr/bin/env python3
"""What the tally (erpl_mc_tally_*) costs, on its own and inside a run.  Recorded, not asserted.  Every GPU step runs in a child
process of its own under a time limit; the first one that fails ends the script.

  add     erpl_mc_tally_add on one window of `--columns` flown columns (default 1 048 576, one DEVICE_CHUNK; planar flights, so
          that nearly every sample is valid and tallied): HIP events, warm, median of 5.  Two specs - the defaults, and 8
          rows of 1024 bins with thresholds, two zones, a 64 x 64 grid and k = 64 - each into an EMPTY tally (every value is
          a candidate for the extremes: the lists overflow and the rows are scanned) and into a FILLED one (the steady state
          of a run: the k-th held value is the admission threshold).  Bytes of summary read = 8 x columns x distinct rows, over
          that time, beside the HBM copy rate of MI355X_MICROARCH.md.  `--variants` lists experiment builds of the library
          (name=path) measured the same way: the rejected forms of the accumulator fold and of the grid counts.
  run     run_monte_carlo_tally of this tree against run_monte_carlo_device of the PARENT commit (`--parent`: a checkout of it
          with its library built) at `--samples` flights (default 4 x 2^20), alternating, `--repeats` times each: samples/s and
          peak device memory (torch.cuda.max_memory_allocated) of both; the spread of the parent's own repeats is what a
          difference has to be read against.  `--run-name` keeps a second size beside the first (the memory of the two
          at a size where the pipeline is full).
  long    one run_monte_carlo_tally of `--long-samples` flights: wall time and both memory readings (the state, the peak).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = {"measured_copy": 6.29, "spec": 8.0}

PRELUDE = r"""
import json, os, statistics, sys, time
sys.path.insert(0, %(tree)r)
import numpy as np
import torch
from erpl_monte_carlo_sim_amd import _abi, analysis, models
from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
IC = {"position": [0.0, 0.0, 10.0], "velocity": [0, 0, 0.0], "attitude": [0.0, -np.pi / 2 + 0.02, 0.0],
      "angular_velocity": [0.0, 0.0, 0.0]}
mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
"""

ADD = PRELUDE + r"""
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
n, lib = %(columns)d, %(lib)r
run = mc.run_monte_carlo_device(dict(IC), n, planar=True)
summ, status = run["summary"].contiguous(), run["status"].contiguous()
eng = TrajectoryEngine(torch.device("cuda", 0), lib_path=lib)
R = analysis.ROW_NAMES
heavy_rows = ["apogee_altitude", "range", "flight_time", "max_speed", "impact_x", "impact_y", "apogee_time", "final_vz"]
heavy_ranges = [(0, 80000.0), (0, 200000.0), (0, 600.0), (0, 2000.0), (-2e5, 2e5), (-2e5, 2e5), (0, 300.0), (-500.0, 500.0)]
specs = {"defaults": analysis.tally_spec(),
         "eight_rows_zones_k64": analysis.tally_spec(rows=heavy_rows, ranges=heavy_ranges, bins=1024, k=64, grid_bins=64,
                                                     thresholds=[[r[1] * 0.5, r[1] * 0.9] for r in heavy_ranges],
                                                     zones=[[[-2000, -2000], [3000, -1000], [1000, 4000]],
                                                            [[0, 0], [50000, 0], [50000, 50000], [0, 50000]]])}
out = {"columns": n, "valid": int(run["n_samples"]), "library": %(libname)r}
for name, spec in specs.items():
    rows = set(spec.rows[:spec.n_rows]) | {0, 4, 5, spec.row_x, spec.row_y}
    nbytes = 8 * n * len(rows) + 4 * n
    _, state = eng.tally_new(spec)
    filled = state.clone()
    eng.tally_add(spec, filled, summ, status, first_id=0)
    torch.cuda.synchronize()
    for mode in ("empty", "filled"):
        ms = []
        for it in range(3 + 5):
            state.copy_(filled) if mode == "filled" else state.zero_()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            eng.tally_add(spec, state, summ, status, first_id=n if mode == "filled" else 0)
            t1.record()
            t1.synchronize()
            if it >= 3:
                ms.append(t0.elapsed_time(t1))
        med = statistics.median(ms)
        out[name + "_" + mode] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "calls": 5, "summary_bytes_read": nbytes,
                                  "read_TB_per_s": nbytes / (1e-3 * med) / 1e12,
                                  "share_of_measured_hbm_copy_rate": nbytes / (1e-3 * med) / 1e12 / %(hbm)r}
    out[name + "_state_bytes"] = int(state.numel()) * 8
print("RESULT " + json.dumps(out))
"""

RUN = PRELUDE + r"""
n, what = %(samples)d, %(what)r
fly = (lambda m: mc.run_monte_carlo_tally(dict(IC), m)) if what == "tally" else (lambda m: mc.run_monte_carlo_device(dict(IC), m))
fly(1 << 16)                                  # warm: the context, the workspaces, the allocator
torch.cuda.synchronize()
torch.cuda.empty_cache()
torch.cuda.reset_peak_memory_stats()
t0 = time.time()
out = fly(n)
torch.cuda.synchronize()
wall = time.time() - t0
res = {"what": what, "samples": n, "wall_s": wall, "samples_per_s": n / wall,
       "peak_memory_bytes": int(torch.cuda.max_memory_allocated()), "n_valid": int(out["n_samples"])}
if what == "tally":
    res["state_bytes"] = int(out["state"].numel()) * 8
    res["range_exceedance_of_the_largest_held"] = out["rows"]["range"]["largest"][:3]
print("RESULT " + json.dumps(res))
"""


def child(code, limit):
    """One GPU step: a fresh process under a time limit.  Returns its RESULT line; a failure ends the script."""
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", code], capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"a GPU step ended with status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["add", "run", "long"], choices=["add", "run", "long"])
    ap.add_argument("--columns", type=int, default=1 << 20)
    ap.add_argument("--variants", nargs="*", default=[], help="name=path of experiment builds of the library")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--samples", type=int, default=4 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--run-name", default="run", help="key of the `run` part in the record: several sizes side by side")
    ap.add_argument("--long-samples", type=int, default=1 << 28)
    ap.add_argument("--out", default="profiles/tally_bench.json")
    args = ap.parse_args()
    report = {"what": "erpl_mc_tally_add: HIP-event milliseconds per call, warm, median of 5; runs: wall seconds of one call in a "
                      "fresh process behind a 65 536-flight warm-up, peak = torch.cuda.max_memory_allocated",
              "guide_hbm_TB_per_s": HBM_TBS}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            report.update(json.load(fh))     # parts measured in an earlier call stay
    if "add" in args.parts:
        report["add"] = {}
        for name, lib in [("product", None)] + [tuple(v.split("=", 1)) for v in args.variants]:
            r = child(ADD % {"tree": ROOT, "columns": args.columns, "lib": lib and os.path.abspath(lib), "libname": lib or "product",
                             "hbm": HBM_TBS["measured_copy"]}, 300)
            report["add"][name] = r
            print(name, json.dumps(r), flush=True)
    if "run" in args.parts:
        if not args.parent:
            sys.exit("--parent: the comparison is against run_monte_carlo_device of the parent commit")
        runs = {"parent_device": [], "tally": []}
        for _ in range(args.repeats):
            for key, tree, what in (("parent_device", os.path.abspath(args.parent), "device"), ("tally", ROOT, "tally")):
                r = child(RUN % {"tree": tree, "samples": args.samples, "what": what}, 300)
                runs[key].append(r)
                print(key, json.dumps(r), flush=True)
        summary = {}
        for key, rs in runs.items():
            rate = [r["samples_per_s"] for r in rs]
            summary[key] = {"samples_per_s_median": statistics.median(rate), "samples_per_s_min": min(rate), "samples_per_s_max": max(rate),
                            "spread_over_median": (max(rate) - min(rate)) / statistics.median(rate),
                            "peak_memory_bytes": max(r["peak_memory_bytes"] for r in rs)}
        summary["tally_over_parent_median"] = summary["tally"]["samples_per_s_median"] / summary["parent_device"]["samples_per_s_median"]
        report[args.run_name] = {"samples": args.samples, "repeats": args.repeats, "runs": runs, "summary": summary}
        print(json.dumps(summary), flush=True)
    if "long" in args.parts:
        limit = 120 + args.long_samples // 1_000_000
        report["long"] = child(RUN % {"tree": ROOT, "samples": args.long_samples, "what": "tally"}, limit)
        print("long", json.dumps(report["long"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
