#!/usr/bin/env python3
"""erpl_mc_impact_density_weighted against erpl_mc_impact_density on the same points, interleaved in one process, and
against scipy.stats.gaussian_kde(weights=) in one host process.

The points: `--points` counted samples of a correlated Gaussian cloud (every sample counted), the weights
floor(2^40 exp(l - l_max)) with l = -Exp(4), as a strongly changed law gives them; `--nodes` x `--nodes` nodes.  One warm-up
round, then `--rounds` timed rounds; a round runs the four calls one after the other - weighted and unweighted, each without
the sample pass (levels=()) and with it (the default levels) - every window closed by a device synchronise (the calls
return when the result is filled).  Reported: the median of every call, pairs per second of the node pass (nodes * m over
the call without the sample pass) and of the sample pass (m * m over the difference), the ratio weighted / unweighted of both
rates, and next to it the unweighted call's own run-to-run spread ((max - min) / median over the rounds).  Whole-call
figures: launches, the moment passes, the selection and the host's two waits are inside.
scipy: gaussian_kde(points, weights=)(nodes) on `--scipy-nodes` nodes, EXTRAPOLATED linearly to all nodes; the same answer
first."""
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

from erpl_monte_carlo_sim_amd import _abi                       # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine    # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms),
            "spread": (max(ms) - min(ms)) / statistics.median(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-nodes", type=int, default=32)
    ap.add_argument("--out", default="profiles/density_w_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = TrajectoryEngine(dev)
    m, nodes = args.points, (args.nodes, args.nodes)
    rng = np.random.default_rng(20)
    z = rng.standard_normal((2, m))
    summ = np.zeros((_abi.SUMMARY_DIM, m))
    summ[_abi.SUM_IMPACT_X] = 1500.0 + 300.0 * z[0]
    summ[_abi.SUM_IMPACT_Y] = -800.0 + 120.0 * (0.9 * z[0] + math.sqrt(1.0 - 0.81) * z[1])
    l = -rng.exponential(4.0, m)
    W = np.maximum(np.floor(np.ldexp(np.exp(l - l.max()), 40)), 1.0).astype(np.int64)   # every sample counted
    s, w = torch.from_numpy(summ).to(dev), torch.from_numpy(W).to(dev)
    calls = {"weighted_map": lambda: eng.impact_density_weighted(s, w, nodes=nodes, levels=()),
             "weighted_map_and_regions": lambda: eng.impact_density_weighted(s, w, nodes=nodes),
             "unweighted_map": lambda: eng.impact_density(s, nodes=nodes, levels=()),
             "unweighted_map_and_regions": lambda: eng.impact_density(s, nodes=nodes)}
    ms = {k: [] for k in calls}
    last = {}
    for r in range(args.rounds + 1):
        for name, fn in calls.items():
            t, last[name] = timed(fn)
            if r:   # round 0 warms up
                ms[name].append(t)
    assert last["weighted_map"]["count"] == m == last["unweighted_map"]["count"]
    report = {"what": "wall milliseconds per call, warm, median over interleaved rounds in one process; whole-call figures",
              "points": m, "nodes": list(nodes), "ess": last["weighted_map"]["ess"]}
    for name in calls:
        report[name] = summary(ms[name])
    grid_pairs, sample_pairs = nodes[0] * nodes[1] * m, m * m
    for kind in ("weighted", "unweighted"):
        a, b = report[kind + "_map"]["median_ms"], report[kind + "_map_and_regions"]["median_ms"]
        report[kind + "_grid_pairs_per_s"] = grid_pairs / (1e-3 * a)
        report[kind + "_sample_pass_ms"] = b - a
        report[kind + "_sample_pairs_per_s"] = sample_pairs / (1e-3 * (b - a))
    report["grid_rate_ratio_weighted_over_unweighted"] = report["weighted_grid_pairs_per_s"] / report["unweighted_grid_pairs_per_s"]
    report["sample_rate_ratio_weighted_over_unweighted"] = report["weighted_sample_pairs_per_s"] / report["unweighted_sample_pairs_per_s"]
    report["unweighted_run_to_run_spread"] = report["unweighted_map"]["spread"]
    # scipy on a share of the nodes: the same answer first, then the time
    from scipy import stats
    got = last["weighted_map"]
    gx, gy = np.meshgrid(got["grid_x"], got["grid_y"], indexing="ij")
    pick = np.arange(0, gx.size, max(1, gx.size // args.scipy_nodes))[:args.scipy_nodes]
    kde = stats.gaussian_kde(summ[[_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y]], weights=W.astype(np.float64))
    t0 = time.perf_counter()
    ref = kde(np.vstack([gx.ravel()[pick], gy.ravel()[pick]]))
    sec = time.perf_counter() - t0
    body = ref >= 1e-12 * ref.max()
    err = float(np.abs(got["density"].ravel()[pick][body] / ref[body] - 1.0).max())
    assert err < 1e-8, err
    report["scipy"] = {"nodes_timed": int(len(pick)), "seconds": sec, "EXTRAPOLATED_seconds_all_nodes": sec * gx.size / len(pick),
                       "EXTRAPOLATED_over_weighted_map": 1e3 * sec * gx.size / len(pick) / report["weighted_map"]["median_ms"],
                       "max_rel_difference_on_body_nodes": err}
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
