#!/usr/bin/env python3
"""erpl_mc_reweight (TrajectoryEngine.reweight) at (columns, law rows, outcome rows) = (131 072, 4, 3) and (1 048 576, 17, 3),
thresholds on one row, five quantiles.  Recorded, not asserted; writes profiles/reweight_bench.json.

  call            wall-clock milliseconds of the whole call, warm, median of `--calls` after `--warmup` calls: the call ends in
                  its own stream synchronise (it hands the result back on the host), so the host clock around it is the time
                  a user waits
  restatement     tests/reweight_ref.py (NumPy, one host process) on the same inputs, once: the yardstick
  --profile       three calls of each shape and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`
  --kernel-stats  the kernel_stats.csv of that run: per kernel its calls and average time, the bytes its launches read and
                  write (from the shapes) over that time and as a share of the HBM copy rate of MI355X_MICROARCH.md (6.29
                  TB/s measured); the finishing and scan kernels move a few KB - they are launch-bound, and are marked so
"""
import argparse
import csv
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

from erpl_monte_carlo_sim_amd import _abi                            # noqa: E402
from erpl_monte_carlo_sim_amd.simulator import shared_engine         # noqa: E402

HBM_COPY_TBS = 6.29
SHAPES = ((131072, 4, 3), (1048576, 17, 3))
QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)
ROWS = (_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME)


def make_inputs(n, n_law, seed=3):
    """n_law law rows, every fourth one uniform, mild changes (an ESS share of some 0.5 at 4 rows), and a summary."""
    rng = np.random.default_rng(seed)
    kinds = [_abi.DESIGN_UNIFORM if r % 4 == 3 else _abi.DESIGN_NORMAL for r in range(n_law)]
    law = [(0.0, 0.9) if k == _abi.DESIGN_UNIFORM else (0.05 * (r % 3 - 1), 0.95) for r, k in enumerate(kinds)]
    factors = np.stack([rng.uniform(size=n) if k == _abi.DESIGN_UNIFORM else rng.normal(size=n) for k in kinds])
    summary = rng.normal(size=(_abi.SUMMARY_DIM, n)) * 50.0 + 3000.0
    return factors, kinds, law, summary


def kernel_bytes(n, n_law, n_rows):
    """Bytes the launches of ONE call read and write, per kernel name, from the shapes (no mask; logw and weights kept)."""
    return {"rw_logw": 8 * n * (n_law + n_rows) + 8 * n, "rw_weights": 16 * n,
            "rw_rows<false>": 16 * n * n_rows, "rw_rows<true>": 16 * n * n_rows, "rw_hist": 8 * 16 * n * n_rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --profile run under rocprofv3, merged into --out")
    ap.add_argument("--profile-shape", type=int, default=1, help="index into SHAPES of the --profile run")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--out", default="profiles/reweight_bench.json")
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as fh:
            report = json.load(fh)
        n, n_law, n_rows = SHAPES[args.profile_shape]
        per_call = kernel_bytes(n, n_law, n_rows)
        launches = {"rw_hist": 8}
        kernels = {}
        with open(args.kernel_stats) as fh:
            for rec in csv.DictReader(fh):
                name = rec["Name"]
                if "rw_" not in name:
                    continue
                short = name[name.index("rw_"):].split("(")[0].replace("ILb0EEEv", "<false>(").replace("ILb1EEEv", "<true>(").split("(")[0]
                short = short.split("ENS_")[0].split("EPNS_")[0]                 # a mangled name: what follows the function's
                entry = {"calls": int(rec["Calls"]), "average_us": float(rec["AverageNs"]) / 1e3, "min_us": float(rec["MinNs"]) / 1e3}
                key = next((k for k in per_call if short.replace(" ", "").startswith(k.replace(" ", ""))), None)
                if key is not None:
                    entry["bytes_per_launch"] = per_call[key] // launches.get(key, 1)
                    entry["TB_per_s"] = entry["bytes_per_launch"] / (entry["average_us"] * 1e-6) / 1e12
                    entry["share_of_measured_hbm_copy_rate"] = entry["TB_per_s"] / HBM_COPY_TBS
                else:
                    entry["bound"] = "launch: one to four workgroups over a few KB of partials"
                kernels[short] = entry
        report["kernels"] = {"shape": {"columns": n, "law_rows": n_law, "rows": n_rows}, "source": "rocprofv3 --kernel-trace --stats, a run of its own",
                             "per_kernel": kernels}
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1)
        print(json.dumps(report["kernels"], indent=1))
        return
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = shared_engine(dev)
    thresholds = {_abi.SUM_RANGE: [2950.0, 3000.0, 3050.0]}
    report = {"what": "wall-clock milliseconds per call of TrajectoryEngine.reweight (it ends in its own stream synchronise), warm, "
                      "median; the NumPy restatement of the tests on the same inputs, once", "guide_hbm_copy_TB_per_s": HBM_COPY_TBS, "shapes": []}
    shapes = (SHAPES[args.profile_shape],) if args.profile else SHAPES
    for n, n_law, n_rows in shapes:
        factors, kinds, law, summary = make_inputs(n, n_law)
        f, s = torch.from_numpy(factors).to(dev), torch.from_numpy(summary).to(dev)
        call = lambda: eng.reweight(f, kinds, law, s, rows=ROWS[:n_rows], thresholds=thresholds, quantiles=QUANTILES)
        if args.profile:
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            continue
        for _ in range(args.warmup):
            out = call()
        ms = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call()
            ms.append(1e3 * (time.perf_counter() - t0))
        rec = {"columns": n, "law_rows": n_law, "rows": n_rows, "thresholds": 3, "quantiles": len(QUANTILES), "launches": 24,
               "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": args.calls,
               "bytes_of_all_passes": sum(kernel_bytes(n, n_law, n_rows).values()), "ess": out["ess"], "count": out["count"]}
        rec["TB_per_s_of_the_call"] = rec["bytes_of_all_passes"] / (1e-3 * rec["median_ms"]) / 1e12
        if not args.no_restatement:
            import reweight_ref as R
            t0 = time.perf_counter()
            ref = R.reweight(factors, kinds, law, summary, rows=ROWS[:n_rows], thresholds=thresholds, quantiles=QUANTILES)
            rec["numpy_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
            rec["numpy_over_native"] = rec["numpy_restatement_ms"] / rec["median_ms"]
            rec["same_integers"] = ref["sum_w"] == out["sum_w"] and all(
                ref["rows"][r]["quantiles"] == out["rows"][r]["quantiles"] and ref["rows"][r]["exceed_w"] == out["rows"][r]["exceed_w"]
                for r in ROWS[:n_rows])
        report["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    if args.profile:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
