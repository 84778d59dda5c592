#!/usr/bin/env python3
"""TrajectoryEngine.compare (erpl_mc_compare) on two synthetic runs of the size of a default run's valid population, against
the NumPy yardstick of tests/compare_ref.py in one host process.

Two cases, P = 999 permutations, three rows (apogee, range, flight time: normal values, B's range moved by 0.05 sigma):

  27 037 + 27 037   the valid share of a default 1 048 576-sample run, with the bivariate energy test on the impact points
  131 072 + 131 072 the rank tests alone (xy=None)

Per case, warm (`--warmup` calls), median of `--calls`, every window closed by a device synchronise (the call returns when the
result is filled).  From whole-call times: pair-permutations per second (N^2 (P + 1) over the difference of the call with and
without the bivariate test) and member-permutations per second (R N (P + 1) over the rank-only call), and their share of the
fp64 vector ISSUE peak (one fp64 wave-instruction per 4 cycles per SIMD, 1 024 SIMDs, 2.4 GHz) at `--valu-per-pair` /
`--valu-per-member` vector instructions each (counted with tools/isa_mix.py in the listings of erpl_cmp_pairs and
erpl_cmp_walk: DESIGN.md section 8.10).  Launches, the sorts, the label passes and the host's waits are inside these figures;
the split per pass comes from a kernel trace in a run of its own.

NumPy: compare_ref.rank_stats per row and permutation and compare_ref.energy_f64_all (float64, one matrix product) on
`--numpy-permutations` permutations and, for the distances, `--numpy-points` points, EXTRAPOLATED linearly in P and
quadratically in N."""
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

from erpl_monte_carlo_sim_amd import _abi, flatten, models   # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine  # noqa: E402

ISSUE_PEAK = 1024 * 2.4e9 / 4 * 64   # fp64 lane-instructions per second: 16 lanes per clock per SIMD
ROWS = (_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME)


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


def make_run(m, seed, moved):
    rng = np.random.default_rng(seed)
    summ = np.zeros((_abi.SUMMARY_DIM, m))
    summ[_abi.SUM_APOGEE_ALT] = rng.normal(9000.0, 400.0, m)
    summ[_abi.SUM_RANGE] = rng.normal(2500.0 + (0.05 * 600.0 if moved else 0.0), 600.0, m)
    summ[_abi.SUM_FLIGHT_TIME] = rng.normal(90.0, 4.0, m)
    summ[_abi.SUM_IMPACT_X] = rng.normal(1500.0, 300.0, m)
    summ[_abi.SUM_IMPACT_Y] = rng.normal(-800.0, 120.0, m)
    return summ


def numpy_leg(a, b, args):
    """The yardstick on a share of the work: seconds, and the extrapolation to the whole case."""
    import compare_ref as ref
    m_a, m_b = a.shape[1], b.shape[1]
    labs = [ref.identity(m_a, m_b)] + [ref.labels(0, p, m_a, m_b) for p in range(args.numpy_permutations)]
    t0 = time.perf_counter()
    for r in ROWS:
        rk = ref.Ranked(np.r_[a[r], b[r]])
        for lab in labs:
            ref.rank_stats(rk, lab)
    rank_s = time.perf_counter() - t0
    k = min(args.numpy_points, m_a, m_b)
    x, y = np.r_[a[_abi.SUM_IMPACT_X, :k], b[_abi.SUM_IMPACT_X, :k]], np.r_[a[_abi.SUM_IMPACT_Y, :k], b[_abi.SUM_IMPACT_Y, :k]]
    small = [ref.identity(k, k)] + [ref.labels(0, p, k, k) for p in range(args.numpy_permutations)]
    t0 = time.perf_counter()
    ref.energy_f64_all(ref.Cloud(x, y, exact=False), small)
    pair_s = time.perf_counter() - t0
    share = (args.permutations + 1) / (args.numpy_permutations + 1)
    return {"numpy_permutations_timed": args.numpy_permutations, "numpy_points_timed": 2 * k, "numpy_rank_s": rank_s,
            "numpy_pair_s": pair_s, "numpy_rank_s_extrapolated": rank_s * share,
            "numpy_pair_s_extrapolated": pair_s * share * ((m_a + m_b) / (2.0 * k)) ** 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bivariate-points", type=int, default=27037)
    ap.add_argument("--rank-points", type=int, default=131072)
    ap.add_argument("--permutations", type=int, default=999)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--numpy-permutations", type=int, default=9)
    ap.add_argument("--numpy-points", type=int, default=2048)
    ap.add_argument("--valu-per-pair", type=float, default=1.45)
    ap.add_argument("--valu-per-member", type=float, default=86.0)
    ap.add_argument("--out", default="profiles/compare_native_vs_numpy.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = TrajectoryEngine(dev)
    eng.set_config(flatten.config_from_objects(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere()))
    P, R = args.permutations, len(ROWS)
    report = {"what": "wall milliseconds per call of TrajectoryEngine.compare, warm, median; synthetic normal rows and impact "
                      "points, every sample counted; NumPy: tests/compare_ref.py in one host process, timed on a share and "
                      "extrapolated; the rates are whole-call figures",
              "permutations": P, "rows": R, "valu_instructions_per_pair_permutation": args.valu_per_pair,
              "valu_instructions_per_member_permutation": args.valu_per_member,
              "fp64_issue_peak_lane_instructions_per_s": ISSUE_PEAK, "cases": []}
    for m, bivariate in ((args.bivariate_points, True), (args.rank_points, False)):
        a, b = make_run(m, 1, False), make_run(m, 2, True)
        da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        N = 2 * m
        row = {"m_a": m, "m_b": m, "bivariate": bivariate}
        row["ranks_only"] = wall(lambda: eng.compare(da, db, rows=ROWS, xy=None, permutations=P, knots=0), args.warmup, args.calls)
        row["member_permutations_per_s"] = R * N * (P + 1) / (1e-3 * row["ranks_only"]["median_ms"])
        row["rank_share_of_issue_peak"] = row["member_permutations_per_s"] * args.valu_per_member / ISSUE_PEAK
        if bivariate:
            row["all_tests"] = wall(lambda: eng.compare(da, db, rows=ROWS, permutations=P, knots=0), args.warmup, args.calls)
            pair_ms = row["all_tests"]["median_ms"] - row["ranks_only"]["median_ms"]
            row["pair_pass_ms"] = pair_ms
            row["pair_permutations_per_s"] = float(N) * N * (P + 1) / (1e-3 * pair_ms)
            row["pair_share_of_fp64_issue_peak"] = row["pair_permutations_per_s"] * args.valu_per_pair / ISSUE_PEAK
            out = eng.compare(da, db, rows=ROWS, permutations=P, knots=0)
            row["p_values"] = {"range_ks": out["row"][1]["ks"]["p_value"], "energy": out["energy"]["p_value"]}
        row.update(numpy_leg(a, b, args))
        total = row["numpy_rank_s_extrapolated"] + (row["numpy_pair_s_extrapolated"] if bivariate else 0.0)
        row["numpy_over_native"] = 1e3 * total / row["all_tests" if bivariate else "ranks_only"]["median_ms"]
        report["cases"].append(row)
        print(json.dumps(row), flush=True)
        del da, db
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
