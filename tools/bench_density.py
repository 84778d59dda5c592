#!/usr/bin/env python3
"""analysis.impact_probability (erpl_mc_analyze + erpl_mc_impact_density) on the impact points of real f64_fast runs of
Set S, against scipy.stats.gaussian_kde in one host process.

Per run size the summary is integrated once; its valid population is one size, and the same tensors tiled until the
counted points pass each `--targets` value give the others (tiles repeat impact points exactly: the arithmetic per pair is
the same, the thresholds tie).  Per size, warm (`--warmup` calls), median of `--calls`, every window closed by a device
synchronise (the call returns when the result is filled):

  map          nodes only (levels=()): 128 x 128 (the default) and 256 x 256 nodes
  map+regions  the defaults (levels 50 / 90 / 99 %), which add the pass over all pairs of counted samples (m * m)
  pair rate    pair evaluations per second of the two passes from whole-call times - nodes * m over the 256 x 256 map call,
               m * m over the difference map+regions - map at 128 x 128 - and their share of the fp64 vector ISSUE peak: one
               fp64 wave-instruction per 4 cycles per SIMD, 1 024 SIMDs, 2.4 GHz, `--valu-per-pair` vector instructions per
               pair (counted in the ISA listing of erpl_dens_pairs: DESIGN.md section 8.5).  Whole-call figures: launches,
               the moment passes and the host's two waits are inside.
  scipy        gaussian_kde(points)(nodes) in one host process on `--scipy-nodes` nodes of the 128 x 128 grid, EXTRAPOLATED
               linearly to all nodes (and to the m points for the density at the samples); the same answer first
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

from erpl_monte_carlo_sim_amd import _abi, analysis, flatten, models, sampling   # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine                     # noqa: E402

EXAMPLE_IC = {"position": [0.0, 0.0, 10.0], "velocity": [0, 0, 0.0], "attitude": [0.0, -1.5507963267948966, 0.0],
              "angular_velocity": [0.0, 0.0, 0.0]}
ISSUE_PEAK = 1024 * 2.4e9 / 4 * 64   # fp64 lane-instructions per second: 16 lanes per clock per SIMD


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


def scipy_leg(eng, s, t, args):
    """gaussian_kde on a stride of the default grid's nodes: seconds, the extrapolations, and the agreement."""
    from scipy import stats
    got = analysis.impact_probability(s, t, engine=eng, levels=())
    why = eng.analyze(s, t, rows=[], quantiles=[], reasons=True)[1]
    xy = s[[_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y]][:, why == 0].cpu().numpy()
    xy = xy[:, np.isfinite(xy[0]) & np.isfinite(xy[1])]
    assert xy.shape[1] == got["count"]
    gx, gy = np.meshgrid(got["grid_x"], got["grid_y"], indexing="ij")
    nodes = gx.size
    pick = np.arange(0, nodes, max(1, nodes // args.scipy_nodes))[:args.scipy_nodes]
    kde = stats.gaussian_kde(xy)
    t0 = time.perf_counter()
    ref = kde(np.vstack([gx.ravel()[pick], gy.ravel()[pick]]))
    sec = time.perf_counter() - t0
    dev = got["density"].ravel()[pick]
    body = ref >= 1e-12 * ref.max()
    err = float(np.abs(dev[body] / ref[body] - 1.0).max())
    assert err < 1e-8, err   # the same answer first
    per_pair = sec / (len(pick) * xy.shape[1])
    return {"scipy_nodes_timed": int(len(pick)), "scipy_s": sec, "scipy_s_per_pair": per_pair,
            "scipy_s_extrapolated_128x128": per_pair * 128 * 128 * xy.shape[1],
            "scipy_s_extrapolated_256x256": per_pair * 256 * 256 * xy.shape[1],
            "scipy_s_extrapolated_at_the_samples": per_pair * xy.shape[1] * xy.shape[1],
            "max_rel_difference_on_body_nodes": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--targets", type=int, nargs="+", default=[100000, 1000000],
                    help="counted points to tile every run up to (a run that has them already is not tiled)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scipy-nodes", type=int, default=32)
    ap.add_argument("--valu-per-pair", type=float, default=28.5)
    ap.add_argument("--out", default="profiles/density_native_vs_scipy.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    rocket, motor, atm, wm = models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel()
    eng = TrajectoryEngine(dev)
    eng.set_config(flatten.config_from_objects(rocket, motor, atm))
    report = {"what": "wall milliseconds per call of analysis.impact_probability, warm, median; Set S f64_fast impact points, "
                      "the filter of erpl_mc_analyze as the mask; scipy: one host process, timed on scipy_nodes_timed nodes "
                      "and extrapolated linearly; pair rates are whole-call figures",
              "valu_instructions_per_pair": args.valu_per_pair, "fp64_issue_peak_lane_instructions_per_s": ISSUE_PEAK,
              "sizes": []}
    seen = set()
    for n in args.sizes:
        db = sampling.synthetic_dispersions(n, rocket, motor, wm, EXAMPLE_IC, dev, precision=_abi.PREC_F64_FAST, seed=1234,
                                            engine=eng)
        summ, status = eng.run(db)
        torch.cuda.synchronize()
        del db
        base = analysis.impact_probability(summ, status, engine=eng, levels=(), nodes=(2, 2))["count"]
        tiles = sorted({1} | {-(-target // base) for target in args.targets if target > base})
        for tile in tiles:
            s = summ.repeat(1, tile).contiguous() if tile > 1 else summ
            t = status.repeat(tile).contiguous() if tile > 1 else status
            m = base * tile
            if m in seen:
                continue
            seen.add(m)
            row = {"run_samples": n, "tile": tile, "n": int(s.shape[1]), "count": m}
            for name, nodes in (("128x128", (128, 128)), ("256x256", (256, 256))):
                row["map_" + name] = wall(lambda: analysis.impact_probability(s, t, engine=eng, nodes=nodes, levels=()),
                                          args.warmup, args.calls)
                row["map_and_regions_" + name] = wall(lambda: analysis.impact_probability(s, t, engine=eng, nodes=nodes),
                                                      args.warmup, args.calls)
            grid_pairs = 256 * 256 * m
            row["grid_pairs_per_s"] = grid_pairs / (1e-3 * row["map_256x256"]["median_ms"])
            sample_ms = row["map_and_regions_128x128"]["median_ms"] - row["map_128x128"]["median_ms"]
            row["sample_pass_ms"] = sample_ms
            row["sample_pairs_per_s"] = m * m / (1e-3 * sample_ms)
            for k in ("grid", "sample"):
                row[k + "_share_of_fp64_issue_peak"] = row[k + "_pairs_per_s"] * args.valu_per_pair / ISSUE_PEAK
            row.update(scipy_leg(eng, s, t, args))
            row["scipy_over_native_128x128_map"] = 1e3 * row["scipy_s_extrapolated_128x128"] / row["map_128x128"]["median_ms"]
            report["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del s, t
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
