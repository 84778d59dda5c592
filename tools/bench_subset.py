#!/usr/bin/env python3
"""The five calls of erpl_mc_subset_* at the primitive tensor of a K = 100 run (17 + 3 K + 2 = 319 rows) and `--chains`
chains (default 131 072) of `--steps` steps, and one rare_event of the planar set at a range threshold near P = 1e-6.
Recorded, not asserted.

  calls        HIP-event time of each call on its stream, warm, buffers allocated before: median of `--calls` after
               `--warmup` warm-up calls
  bytes        what the algorithm has to move, from the shapes: the gather reads and writes chains * (319 + 16 + 1) * 8 + 4
               bytes per column (and 64-byte sectors where it reads), the commit reads two and writes one of them; over the
               time, beside the HBM copy rate of MI355X_MICROARCH.md (6.29 TB/s measured)
  proposal     fp64 operations per value counted from the source (Philox is integer work and is not counted): PPND16 central
               branch 2 x 7 FMA + 4, tails a log and a sqrt more, 3 for rho x + s xi - about 40; over the time, beside the
               78.65 TFLOP/s fp64 vector peak.  A share, not a kernel counter.
  rare_event   a planar tally run of `--tally-flights` flights whose filter drops ranges beyond `--max-range` (the freak mode
               of the planar set, which chains cannot reach: DESIGN.md section 8.15) picks the threshold (its k-th largest held range), then one
               rare_event(target=that) - wall time, evaluations, P and c.o.v. - against the flights direct Monte Carlo needs
               for the same c.o.v., (1 - P) / (P cov^2), at the tally run's measured flights per second (EXTRAPOLATED)
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from erpl_monte_carlo_sim_amd import _abi, analysis, models, sampling      # noqa: E402
from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer        # noqa: E402
from erpl_monte_carlo_sim_amd.simulator import shared_engine               # noqa: E402

K = 100
HBM_TBS = 6.29
FP64_VECTOR_TFLOPS = 78.65
PROPOSAL_FLOP_PER_VALUE = 40
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


def with_bytes(t, nbytes):
    t["bytes"] = int(nbytes)
    t["TB_per_s"] = nbytes / (1e-3 * t["median_ms"]) / 1e12
    t["share_of_measured_hbm_copy_rate"] = t["TB_per_s"] / HBM_TBS
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--tally-flights", type=int, default=1 << 24)
    ap.add_argument("--n-per-level", type=int, default=131072)
    ap.add_argument("--max-range", type=float, default=20000.0)
    ap.add_argument("--skip-run", action="store_true")
    ap.add_argument("--out", default="profiles/subset_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = shared_engine(dev)
    R, C, T = sampling.primitive_rows(K), args.chains, args.steps
    N = C * T
    kinds = [_abi.DESIGN_NORMAL] * (R - 2) + [_abi.DESIGN_UNIFORM] * 2
    report = {"what": "HIP-event milliseconds per call, warm, median; bytes and operations from the shapes", "rows": R, "chains": C,
              "steps": T, "guide": {"hbm_copy_TB_per_s": HBM_TBS, "fp64_vector_TFLOP_per_s": FP64_VECTOR_TFLOPS}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    # the seeds are drawn out of a population of N columns (the gather's permuted reads), the rounds work on blocks of C
    pop = eng.design(kinds, N, 7, kind="random")
    nxt = torch.empty((R, 2 * C), dtype=torch.float64, device=dev)
    summ = torch.rand((16, N), generator=gen, dtype=torch.float64, device=dev) * 1000.0 + 500.0
    summ_nxt = torch.empty((16, 2 * C), dtype=torch.float64, device=dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    status_nxt = torch.empty(2 * C, dtype=torch.int32, device=dev)
    spec = analysis.subset_spec()
    calls = {}
    g = eng.subset_limit_state(spec, summ, status)
    g_nxt = torch.empty(2 * C, dtype=torch.float64, device=dev)
    calls["limit_state"] = with_bytes(event_ms(lambda: eng.subset_limit_state(spec, summ, status, out=g), args.warmup, args.calls),
                                      N * (4 * 8 + 4 + 8))
    gathers = [(pop, nxt[:, :C]), (summ, summ_nxt[:, :C]), (status, status_nxt[:C]), (g, g_nxt[:C])]
    calls["seeds_select_only"] = with_bytes(event_ms(lambda: eng.subset_seeds(g, C), args.warmup, args.calls), N * 8 * 10 + N)
    t_all = event_ms(lambda: eng.subset_seeds(g, C, gathers), args.warmup, args.calls)
    per_col = (R + 16 + 1) * 8 + 4
    calls["seeds_with_gather"] = t_all
    calls["gather"] = with_bytes({"median_ms": t_all["median_ms"] - calls["seeds_select_only"]["median_ms"],
                                  "what": "seeds_with_gather - seeds_select_only (medians)"}, 2 * C * per_col)
    calls["gather"]["sector_bytes"] = int(C * (R + 16 + 1) * 64 + C * 32 + C * per_col)
    cand = torch.empty((R, C), dtype=torch.float64, device=dev)
    pspec = analysis.subset_spec(seed=7, level=1, step=1)
    t = event_ms(lambda: eng.subset_propose(pspec, kinds, 0.8, nxt[:, :C], 0, cand), args.warmup, args.calls)
    t = with_bytes(t, 2 * 8 * R * C)
    t["fp64_TFLOP_per_s"] = PROPOSAL_FLOP_PER_VALUE * R * C / (1e-3 * t["median_ms"]) / 1e12
    t["share_of_fp64_vector_peak"] = t["fp64_TFLOP_per_s"] / FP64_VECTOR_TFLOPS
    calls["propose"] = t
    g_cand = g[:C] + torch.randn(C, generator=gen, dtype=torch.float64, device=dev) * 50.0
    thr = g_nxt[:C].median()
    acc = torch.zeros((), dtype=torch.int64, device=dev)
    triples = [(cand, nxt[:, :C], nxt[:, C:]), (summ[:, :C].contiguous(), summ_nxt[:, :C], summ_nxt[:, C:]),
               (status[:C].contiguous(), status_nxt[:C], status_nxt[C:])]
    calls["commit"] = with_bytes(event_ms(lambda: eng.subset_commit(thr, g_cand, g_nxt[:C], g_nxt[C:], triples, acc), args.warmup, args.calls),
                                 C * (per_col - 4) * 2 + C * 8)
    calls["commit"]["accepted_share"] = float(acc) / (C * (args.warmup + args.calls))
    sel = (torch.rand(N, generator=gen, device=dev) < 0.125).to(torch.uint8)
    calls["chain_stats"] = with_bytes(event_ms(lambda: eng.subset_chain_stats(sel, C, T), args.warmup, args.calls), N)
    report["calls"] = calls
    print(json.dumps(calls), flush=True)
    del pop, nxt, cand, summ, summ_nxt
    torch.cuda.empty_cache()
    if not args.skip_run:
        mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
        mc.run_monte_carlo_device(dict(EXAMPLE_IC), 65536, planar=True, design="random")          # warm-up
        bounds = {"max_range": args.max_range}      # the regular flights: the freak mode beyond it is no business of chains
        tally = analysis.tally_spec(k=64, bounds=bounds)
        run = mc.run_monte_carlo_tally(dict(EXAMPLE_IC), args.tally_flights, tally=tally, planar=True, design="random", seed=4321)
        rng = run["rows"]["range"]
        want = max(1, round(1e-6 * args.tally_flights))       # P counts ALL flights: a dropped one has g = -inf
        x_star = rng["largest"][min(want, len(rng["largest"])) - 1][0]
        direct = {"flights": args.tally_flights, "counted": rng["count"], "bounds": bounds, "largest_20": [v for v, _ in rng["largest"][:20]], "wall_s": run["performance"]["total_time"],
                  "flights_per_s": run["performance"]["simulations_per_second"], "threshold": x_star, "exceeding": want,
                  "probability": want / args.tally_flights, "cov": math.sqrt(1.0 / want)}
        torch.cuda.synchronize()
        t0 = time.time()
        out = mc.rare_event(dict(EXAMPLE_IC), n_per_level=args.n_per_level, p0=0.125, target=x_star, planar=True, seed=1234, bounds=bounds)
        wall = time.time() - t0
        P, cov = out["probability"], out["cov"]
        need = (1 - P) / (P * cov * cov) if P > 0 else float("inf")
        report["rare_event"] = {
            "direct_monte_carlo": direct, "n_per_level": args.n_per_level, "p0": 0.125, "wall_s": wall, "evaluations": out["evaluations"],
            "probability": P, "cov": cov, "interval": out["interval"], "reached": out["reached"], "warnings": out["warnings"],
            "levels": [{k: lv[k] for k in ("threshold", "p", "delta", "gamma", "acceptance")} for lv in out["levels"]],
            "ln_ratio_to_direct": math.log(P / direct["probability"]) if P > 0 else None,
            "direct_flights_for_the_same_cov_EXTRAPOLATED": need,
            "direct_seconds_for_the_same_cov_EXTRAPOLATED": need / direct["flights_per_s"],
            "conditional_inputs": {k: {"mean": v["mean"], "std": v["std"]} for k, v in out["conditional_inputs"].items()}}
        print(json.dumps(report["rare_event"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
