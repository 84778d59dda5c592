#!/usr/bin/env python3
"""The casualty expectation (erpl_mc_casualty) at the debris bench shape, beside erpl_mc_impact_density in the same process
and beside the NumPy restatement tests/casualty_ref.py.

Warm (`--warmup` calls), median of `--calls` host-timed calls, every window closed by a device synchronise:

  footprint      synthetic: `--n` columns x `--nodes` nodes x `--fragments` fragments, one correlated Gaussian cloud per
                 (node, fragment) that moves downrange with the node and widens with the fragment, 2 % of the jobs NaN,
                 impact speeds 5 .. 80 m/s, onto a `--bins` x `--bins` raster with a two-level population
  counts         the call with smooth = 0: e_j, the totals, the split by node and fragment, the hazard map
  smooth         the whole call with smooth = 1; pairs = cells x members of the groups, the pair rate over the time the
                 smoothing adds (smooth - counts)
  density        erpl_mc_impact_density on `--density-n` landing points at the same `--bins` x `--bins` nodes, no levels and
                 no sample pass: its pairs over its whole call - the yardstick, re-measured here, not trusted
  numpy          tests/casualty_ref.py on the first `--host-columns` columns, one process, EXTRAPOLATED by pairs to the shape

`--lib PATH` loads another build of the library (an experiment build, never the product): how the cuts of DESIGN.md 8.19 were
compared.
"""
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

from erpl_monte_carlo_sim_amd import _abi                               # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine             # noqa: E402


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


def footprint(n, nodes, fragments, device, seed=1, spread=1.0):
    """values [5, nodes * fragments, n] on the device; spread scales every cloud (1: a few cells of the bench raster wide)."""
    g = torch.Generator(device=device).manual_seed(seed)
    R = nodes * fragments
    k = (torch.arange(R, device=device) // fragments).double()[:, None]
    f = (torch.arange(R, device=device) % fragments).double()[:, None]
    a, b = (torch.randn((R, n), generator=g, device=device, dtype=torch.float64) for _ in range(2))
    v = torch.empty((_abi.IIP_CH_COUNT, R, n), dtype=torch.float64, device=device)
    sx, sy = spread * (40.0 + 25.0 * f), spread * (30.0 + 15.0 * f)
    v[_abi.IIP_CH_X] = 200.0 + 450.0 * k + sx * a
    v[_abi.IIP_CH_Y] = 40.0 * k - 30.0 * f + 0.4 * sy * a + sy * b
    v[_abi.IIP_CH_VIMPACT] = 5.0 + 75.0 * torch.rand((R, n), generator=g, device=device, dtype=torch.float64)
    v[_abi.IIP_CH_RANGE] = torch.sqrt(v[_abi.IIP_CH_X] ** 2 + v[_abi.IIP_CH_Y] ** 2)
    v[_abi.IIP_CH_TFALL] = 10.0
    lost = torch.rand((R, n), generator=g, device=device) < 0.02
    v[:, lost] = float("nan")
    return v.contiguous()


def setup(args, device):
    F = args.fragments
    frags = [(1.0 + 3.0 * (f % 4), 0.2 + 0.4 * f, 0.05 * 4.0 ** f) for f in range(F)]
    p_fail = np.full(args.nodes, 0.02 / args.nodes)
    ranges = ((-600.0, 450.0 * args.nodes + 600.0), (-1500.0, 1500.0))
    pop = np.full((args.bins, args.bins), 2e-5)
    pop[args.bins // 2:, :] = 1.5e-3
    return frags, p_fail, ranges, torch.as_tensor(pop, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--nodes", type=int, default=16)
    ap.add_argument("--fragments", type=int, default=8)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--density-n", type=int, default=65536)
    ap.add_argument("--host-columns", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    eng = TrajectoryEngine(torch.device("cuda", 0), lib_path=args.lib)
    frags, p_fail, ranges, pop = setup(args, eng.device)
    values = footprint(args.n, args.nodes, args.fragments, eng.device)
    cells = args.bins * args.bins
    res = {"label": args.label, "n": args.n, "nodes": args.nodes, "fragments": args.fragments, "bins": args.bins,
           "jobs": args.n * args.nodes * args.fragments}
    box = {}

    def call(smooth):
        box["out"] = eng.casualty(values, frags, p_fail, pop, ranges, smooth=smooth)

    res["counts"] = wall(lambda: call(False), args.warmup, args.calls)
    res["smooth"] = w = wall(lambda: call(True), args.warmup, args.calls)
    out = box["out"]
    pairs = float(cells) * float(out["groups"][:, 0].sum())
    added = (w["median_ms"] - res["counts"]["median_ms"]) * 1e-3
    w.update({"pairs": pairs, "pairs_per_s_over_added_time": pairs / added, "pairs_per_s_over_whole_call": pairs / (w["median_ms"] * 1e-3),
              "ec": out["ec"], "ec_se": out["ec_se"], "ec_map": out["ec_map"], "ec_smooth": out["ec_smooth"], "mix_mass": out["mix_mass"],
              "lethal": out["lethal"], "missing": out["missing"], "off_grid": out["off_grid"], "q": out["q"],
              "level_area": out["level_area"], "level_area_smooth": out["level_area_smooth"]})

    # the yardstick: the density call at the same nodes, its pair pass alone (no levels, no sample pass)
    g = torch.Generator(device=eng.device).manual_seed(7)
    summ = torch.zeros((_abi.SUMMARY_DIM, args.density_n), dtype=torch.float64, device=eng.device)
    a, b = (torch.randn((args.density_n,), generator=g, device=eng.device, dtype=torch.float64) for _ in range(2))
    summ[_abi.SUM_IMPACT_X], summ[_abi.SUM_IMPACT_Y] = 3000.0 + 900.0 * a, 200.0 + 300.0 * a + 500.0 * b
    dcall = lambda: box.__setitem__("dens", eng.impact_density(summ, nodes=(args.bins, args.bins), levels=()))   # noqa: E731
    d = wall(dcall, args.warmup, args.calls)
    dpairs = float(cells) * float(box["dens"]["count"])
    d.update({"points": int(box["dens"]["count"]), "pairs": dpairs, "pairs_per_s_over_whole_call": dpairs / (d["median_ms"] * 1e-3)})
    res["density"] = d
    res["pair_rate_over_density"] = w["pairs_per_s_over_added_time"] / d["pairs_per_s_over_whole_call"]

    if args.host_columns > 0:
        import casualty_ref
        hc = min(args.host_columns, args.n)
        hv = values[:, :, :hc].cpu().numpy()
        t0 = time.perf_counter()
        want = casualty_ref.casualty(hv, hc, None, frags, p_fail, pop.cpu().numpy(), ranges)
        sec = time.perf_counter() - t0
        hp = float(cells) * float(want["groups"][:, 0].sum())
        res["numpy"] = {"columns_timed": hc, "pairs_timed": hp, "seconds": sec, "EXTRAPOLATED": "by pairs to the whole shape",
                        "seconds_extrapolated_by_pairs": sec / max(hp, 1.0) * pairs}
    line = json.dumps(res, allow_nan=False)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
