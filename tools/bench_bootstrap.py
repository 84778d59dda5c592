#!/usr/bin/env python3
"""erpl_mc_bootstrap (TrajectoryEngine.bootstrap) against the same computation in NumPy, on one synthetic summary per
size: lognormal apogee / range / flight time, 5 % of the samples masked, the default rows and quantiles, B replicates.

  native            wall time of the call, warm (it returns when the result is filled): median of `--calls` after
                    `--warmup` warm-up calls
  kernel split      `--profile` runs three calls per size and nothing else: the run to put under
                    `rocprofv3 --kernel-trace --stats` for the replicate kernel's share (a call with ONE replicate is no
                    measure of the rest: its lone workgroup walks all m draws of every sweep by itself)
  numpy             one process on the host: per replicate the indices from erpl_mc_bootstrap_indices (the library's own
                    host code), x[idx] per row, np.mean, np.std and np.percentile; timed on `--numpy-replicates`
                    replicates and EXTRAPOLATED linearly to B (said so in the report)
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

from erpl_monte_carlo_sim_amd import _abi, analysis, flatten, models      # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine              # noqa: E402

ROWS = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
QUANTILES = [0.05, 0.25, 0.5, 0.75, 0.95]


def tensors(n, seed=7):
    rng = np.random.default_rng(seed)
    summ = rng.normal(size=(_abi.SUMMARY_DIM, n))
    summ[_abi.SUM_APOGEE_ALT] = rng.lognormal(9.0, 0.3, n)
    summ[_abi.SUM_RANGE] = rng.lognormal(7.0, 0.5, n)
    summ[_abi.SUM_FLIGHT_TIME] = rng.lognormal(4.0, 0.3, n)
    mask = (rng.random(n) < 0.05).astype(np.uint8)
    return summ, mask


def wall(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


def numpy_replicates(P, seed, first, count):
    m = P.shape[1]
    out = np.empty((P.shape[0] * (2 + len(QUANTILES)), count))
    pct = [100.0 * q for q in QUANTILES]
    for b in range(count):
        idx = analysis.bootstrap_indices(seed, first + b, m)
        for j in range(P.shape[0]):
            x = P[j, idx]
            k = j * (2 + len(QUANTILES))
            out[k, b], out[k + 1, b] = np.mean(x), np.std(x)
            out[k + 2:k + 2 + len(QUANTILES), b] = np.percentile(x, pct)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--numpy-replicates", type=int, default=50)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="profiles/bootstrap_native_vs_numpy.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = TrajectoryEngine(dev)
    eng.set_config(flatten.config_from_objects(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere()))
    B = args.replicates
    report = {"what": "wall milliseconds per call of TrajectoryEngine.bootstrap, warm; default rows and quantiles, 5 % masked; "
                      "numpy: one host process, timed on numpy_replicates replicates and extrapolated linearly to B",
              "replicates": B, "sizes": []}
    for n in args.sizes:
        summ, mask = tensors(n)
        d_summ, d_mask = torch.from_numpy(summ).to(dev), torch.from_numpy(mask).to(dev)

        def native(b=B, keep=False):
            return eng.bootstrap(d_summ, d_mask, rows=ROWS, quantiles=QUANTILES, replicates=b, seed=11, want_replicates=keep)

        if args.profile:
            for _ in range(3):
                native()
            continue
        P = summ[ROWS][:, mask == 0]
        got = native(args.numpy_replicates, keep=True)
        assert got["count"] == P.shape[1]
        t0 = time.perf_counter()
        ref = numpy_replicates(P, 11, 0, args.numpy_replicates)
        numpy_s = time.perf_counter() - t0
        rep = got["replicate_values"].cpu().numpy()
        err = float(np.max(np.abs(rep - ref) / np.abs(ref)))
        assert err < 1e-11, err   # the same replicates first
        row = {"n": n, "count": got["count"], "native": wall(native, args.warmup, args.calls),
               "numpy_replicates_timed": args.numpy_replicates, "numpy_ms_per_replicate": 1e3 * numpy_s / args.numpy_replicates,
               "numpy_ms_extrapolated_to_B": 1e3 * numpy_s / args.numpy_replicates * B, "max_rel_difference": err}
        row["numpy_over_native"] = row["numpy_ms_extrapolated_to_B"] / row["native"]["median_ms"]
        digits = max(2, ((got["count"] - 1).bit_length() + 7) // 8)   # sweeps per row: two moment sweeps carry two digits
        row["draws_regenerated"] = len(ROWS) * digits * B * got["count"]
        row["draws_per_s_over_the_call"] = row["draws_regenerated"] / (1e-3 * row["native"]["median_ms"])
        report["sizes"].append(row)
        print(json.dumps(row), flush=True)
    if args.profile:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
