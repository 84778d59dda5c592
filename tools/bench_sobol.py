#!/usr/bin/env python3
"""erpl_mc_sobol (TrajectoryEngine.sobol) against the same computation in NumPy, on one synthetic pick-freeze design per
size (n_base, k, B): three output rows of an additive model with one interaction, 2 % of the design rows masked.

  native            HIP-event time of the call on its stream, warm (the call returns when the result is filled): median of
                    `--calls` after `--warmup` warm-up calls
  replicate share   the same with replicates = 0 (population, select, records, estimates) taken off: what the replicate
                    kernel and the one-launch summary over its matrix cost together, as a share of the call
  gathered bytes    what the replicate kernel asks of the record table: per row and replicate m draws, each read once per
                    sweep - 16 bytes (yA, yB) in the mean sweep and 16 + 8 nf bytes in the sweep of a chunk of nf <= 8
                    factors - over the time above; set beside the gather rates of MI355X_MICROARCH.md for a table that
                    fits L2 (16.8 - 18.8 TB/s) or the Infinity Cache (8.6 TB/s)
  numpy             one process on the host: per replicate and row the indices from erpl_mc_bootstrap_indices (the
                    library's own host code), Y[:, idx] and the estimators; timed on `--numpy-replicates` replicates and
                    EXTRAPOLATED linearly to B (said so in the report)
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

ROWS = [_abi.SUM_FIRST_APOGEE_ALT, _abi.SUM_FIRST_APOGEE_TIME, _abi.SUM_RAIL_EXIT_SPEED]
CHUNK = 8   # ERPL_SOBOL_CHUNK
L2_GATHER_TBS, MALL_GATHER_TBS = (16.8, 18.8), 8.6


def design(n, k, seed=7):
    """The three rows [k + 2, n] each (host) and the mask."""
    rng = np.random.default_rng(seed)
    A, B = rng.normal(size=(k, n)), rng.normal(size=(k, n))
    w = rng.uniform(0.5, 2.0, size=(len(ROWS), k))
    rows = np.empty((len(ROWS), k + 2, n))
    for b in range(k + 2):
        X = A if b == 0 else B if b == 1 else np.vstack([A[:b - 2], B[b - 2:b - 1], A[b - 1:]])
        for j in range(len(ROWS)):
            rows[j, b] = 100.0 * (j + 1) + w[j] @ X + X[0] * X[k - 1]
    mask = (rng.random(n) < 0.02).astype(np.uint8)
    return rows, mask


def estimate(Y):
    m = Y.shape[1]
    ya, yb = Y[0], Y[1]
    f0 = (ya.sum() + yb.sum()) / (2 * m)
    cb = yb - f0
    V = (((ya - f0) ** 2).sum() + (cb ** 2).sum()) / (2 * m)
    d = Y[2:] - ya
    return np.concatenate([[f0, V], ((cb * d).sum(axis=1) / m) / V, ((d * d).sum(axis=1) / (2 * m)) / V])


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
    ap.add_argument("--sizes", type=int, nargs="+", default=[16384, 10, 1000, 131072, 32, 1000], help="n_base k B triples")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--numpy-replicates", type=int, default=10)
    ap.add_argument("--out", default="profiles/sobol_native_vs_numpy.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = TrajectoryEngine(dev)
    eng.set_config(flatten.config_from_objects(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere()))
    report = {"what": "HIP-event milliseconds per call of TrajectoryEngine.sobol, warm; three rows, 2 % masked; replicate share = "
                      "(call - call with replicates = 0) / call; gathered bytes = rows * B * m * (16 + sum over chunks of 16 + 8 nf); "
                      "numpy: one host process, timed on numpy_replicates replicates and extrapolated linearly to B",
              "guide_gather_TB_per_s": {"l2_resident": list(L2_GATHER_TBS), "infinity_cache": MALL_GATHER_TBS}, "sizes": []}
    for n, k, B in zip(args.sizes[0::3], args.sizes[1::3], args.sizes[2::3]):
        rows, mask = design(n, k)
        d_summ = torch.zeros((_abi.SUMMARY_DIM, (k + 2) * n), dtype=torch.float64, device=dev)
        for j, r in enumerate(ROWS):
            d_summ[r] = torch.from_numpy(rows[j].reshape(-1)).to(dev)
        d_mask = torch.from_numpy(mask).to(dev)

        def native(b=B, keep=False):
            return eng.sobol(d_summ, n, k, mask=d_mask, rows=ROWS, replicates=b, seed=11, want_replicates=keep)

        nb = args.numpy_replicates
        got = native(nb, keep=True)
        m = int(got["count"][0])
        assert m == int((mask == 0).sum())
        P = rows[:, :, mask == 0]
        t0 = time.perf_counter()
        ref = np.empty((len(ROWS) * (2 + 2 * k), nb))
        for b in range(nb):
            idx = analysis.bootstrap_indices(11, b, m)
            for j in range(len(ROWS)):
                ref[j * (2 + 2 * k):(j + 1) * (2 + 2 * k), b] = estimate(P[j][:, idx])
        numpy_s = time.perf_counter() - t0
        rep = got["replicate_values"].cpu().numpy()
        err = float(np.max(np.abs(rep - ref)))
        assert err < 1e-9, err   # the same replicates first (indices of order one, means of order 100)
        full, bare = event_ms(native, args.warmup, args.calls), event_ms(lambda: native(0), args.warmup, args.calls)
        chunks = [min(CHUNK, k - c) for c in range(0, k, CHUNK)]
        per_draw = 16 + sum(16 + 8 * nf for nf in chunks)
        gathered = len(ROWS) * B * m * per_draw
        rep_ms = full["median_ms"] - bare["median_ms"]
        table_bytes = len(ROWS) * m * (k + 2) * 8
        row = {"n_base": n, "k": k, "B": B, "count": m, "flights": (k + 2) * n, "record_table_bytes": table_bytes,
               "native": full, "native_without_replicates": bare, "replicates_and_summary_ms": rep_ms,
               "replicate_share": rep_ms / full["median_ms"], "sweeps_per_replicate": 1 + len(chunks),
               "gathered_bytes": gathered, "gathered_TB_per_s": gathered / (1e-3 * rep_ms) / 1e12,
               "numpy_replicates_timed": nb, "numpy_ms_per_replicate": 1e3 * numpy_s / nb,
               "numpy_ms_extrapolated_to_B": 1e3 * numpy_s / nb * B, "max_abs_difference": err}
        row["numpy_over_native"] = row["numpy_ms_extrapolated_to_B"] / full["median_ms"]
        report["sizes"].append(row)
        print(json.dumps(row), flush=True)
        del d_summ
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
