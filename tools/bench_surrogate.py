#!/usr/bin/env python3
"""erpl_mc_surrogate (TrajectoryEngine.surrogate) against the yardsticks it is measured by, and what it reads from a flown
Latin hypercube run.  Recorded, not asserted.

  native        warm wall time of the whole call (population, basis, Gram, host Cholesky, residual passes), the input tensors
                on the device: median of `--calls` after `--warmup` warm-up calls, at (n_fit, P) = (27 037, 561), (131 072, 571),
                (1 048 576, 976) - (n_vars, degree, order) = (32, 2, 2), (19, 3, 2), (25, 3, 2), one outcome row, no holdout
  gram          P (P + 1) / 2 * n_fit fused multiply-adds = that many times 2 flops, over the time of the Gram kernels alone
                where `--gram-ms` hands it in (a kernel trace of this program), else over the whole call; beside the fp64
                vector peak of 78.65 TFLOP/s
  torch         Psi @ Psi.T in fp64 on a materialised Psi [P, n_fit] on the same device (HIP events, warm)
  lstsq         numpy.linalg.lstsq of Psi^T on the host, one process; above `--lstsq-max` n_fit P^2 it is extrapolated from
                the largest measured shape by n_fit P^2 and marked so
  predict       erpl_mc_surrogate_predict at `--points` points, (25, 3, 2) model, points per second (HIP events)
  flights       with --flights N: run_monte_carlo_device(N, planar, design='lhs') -> MonteCarloAnalyzer.surrogate (degree 2,
                order 2, holdout 5): r2 / q2 of first-apogee altitude and range, and its first / total indices of five scalar
                primitives beside sobol_indices(design='lhs', n_base=N) on the same five as single-row groups
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

from erpl_monte_carlo_sim_amd import _abi, models                      # noqa: E402
from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer    # noqa: E402
from erpl_monte_carlo_sim_amd.simulator import shared_engine           # noqa: E402

PEAK_TFLOPS = 78.65
SHAPES = ((27037, 32, 2, 2), (131072, 19, 3, 2), (1048576, 25, 3, 2))
EXAMPLE_IC = {"position": [0.0, 0.0, 10.0], "velocity": [0, 0, 0.0], "attitude": [0.0, -np.pi / 2 + 0.02, 0.0],
              "angular_velocity": [0.0, 0.0, 0.0]}


def wall_ms(fn, warmup, calls):
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


def inputs(n, V, dev, seed=5):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    kinds = [_abi.DESIGN_NORMAL if v % 2 == 0 else _abi.DESIGN_UNIFORM for v in range(V)]
    fac = torch.empty((V, n), dtype=torch.float64, device=dev)
    fac[0::2] = torch.randn((len(kinds[0::2]), n), generator=gen, dtype=torch.float64, device=dev)
    fac[1::2] = torch.rand((len(kinds[1::2]), n), generator=gen, dtype=torch.float64, device=dev)
    summ = torch.zeros((_abi.SUMMARY_DIM, n), dtype=torch.float64, device=dev)
    summ[_abi.SUM_APOGEE_ALT] = 3.0 + fac.sum(0) + 0.3 * fac[0] * fac[V - 1] + 0.05 * torch.randn(n, generator=gen, dtype=torch.float64,
                                                                                                 device=dev)
    return kinds, fac, summ


def timing(args, eng, dev):
    report = []
    gram_ms = dict(zip((s[0] for s in SHAPES), args.gram_ms)) if args.gram_ms else {}
    lstsq_ref = None
    for n, V, degree, order in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        kinds, fac, summ = inputs(n, V, dev)
        out = eng.surrogate(fac, kinds, summ, rows=[_abi.SUM_APOGEE_ALT], degree=degree, order=order)
        P = out["n_terms"]
        assert out["n_fit"] == n and out["fit_ok"].all()
        row = {"n_fit": n, "n_vars": V, "degree": degree, "order": order, "P": P, "r2": float(out["r2"][0])}
        row["native_whole_call"] = wall_ms(lambda: eng.surrogate(fac, kinds, summ, rows=[_abi.SUM_APOGEE_ALT], degree=degree, order=order),
                                           args.warmup, args.calls)
        flops = 2.0 * (P * (P + 1) / 2) * n
        row["gram_flops"] = flops
        t = gram_ms.get(n)
        row["gram_kernels_ms"] = t if t is not None else "UNMEASURED"
        row["gram_TFLOPs"] = flops / (1e-3 * t) / 1e12 if t else "UNMEASURED"
        row["gram_share_of_fp64_vector_peak"] = flops / (1e-3 * t) / 1e12 / PEAK_TFLOPS if t else "UNMEASURED"
        row["whole_call_TFLOPs_lower_bound_of_gram"] = flops / (1e-3 * row["native_whole_call"]["median_ms"]) / 1e12
        if args.native_only:     # under a kernel trace: the calls above are what is traced
            report.append(row)
            print(json.dumps(row), flush=True)
            continue
        # torch on a materialised Psi, built from the terms
        terms = out["model"]["terms"]
        Psi = torch.empty((P, n), dtype=torch.float64, device=dev)
        uni = univariate(kinds, fac, degree)
        for t_i, term in enumerate(terms):
            v = torch.ones(n, dtype=torch.float64, device=dev)
            for var, deg in term:
                if var >= 0:
                    v = v * uni[var][deg]
            Psi[t_i] = v
        del uni
        row["torch_Psi_at_PsiT"] = event_ms(lambda: Psi @ Psi.T, args.warmup, args.calls)
        row["torch_TFLOPs_of_the_full_product"] = 2.0 * P * P * n / (1e-3 * row["torch_Psi_at_PsiT"]["median_ms"]) / 1e12
        G_t = (Psi @ Psi.T).cpu().numpy()
        full = eng.surrogate(fac, kinds, summ, rows=[_abi.SUM_APOGEE_ALT], degree=degree, order=order, want_gram=True)
        row["max_rel_difference_to_torch_gram"] = float(np.max(np.abs(full["gram"] - G_t)) / np.max(np.abs(G_t)))
        work = float(n) * P * P
        if work <= args.lstsq_max:
            A = Psi.T.cpu().numpy()
            y = summ[_abi.SUM_APOGEE_ALT].cpu().numpy()
            t0 = time.perf_counter()
            c = np.linalg.lstsq(A, y, rcond=None)[0]
            row["numpy_lstsq_s"] = time.perf_counter() - t0
            row["numpy_lstsq_extrapolated"] = False
            row["max_abs_coefficient_difference_to_lstsq"] = float(np.max(np.abs(c - full["model"]["coefficients"][0])))
            lstsq_ref = (work, row["numpy_lstsq_s"])
            del A
        elif lstsq_ref:
            row["numpy_lstsq_s"] = lstsq_ref[1] * work / lstsq_ref[0]
            row["numpy_lstsq_extrapolated"] = True
        row["lstsq_over_native"] = row["numpy_lstsq_s"] / (1e-3 * row["native_whole_call"]["median_ms"]) if "numpy_lstsq_s" in row else None
        report.append(row)
        print(json.dumps(row), flush=True)
        if (V, degree, order) == (25, 3, 2):
            m = args.points
            gen = torch.Generator(device=dev)
            gen.manual_seed(9)
            X = torch.rand((V, m), generator=gen, dtype=torch.float64, device=dev)
            buf = torch.empty((1, m), dtype=torch.float64, device=dev)
            t = event_ms(lambda: eng.surrogate_predict(out["model"], X, out=buf), args.warmup, args.calls)
            t["points"], t["P"] = m, P
            t["points_per_second"] = m / (1e-3 * t["median_ms"])
            report.append({"predict": t})
            print(json.dumps(t), flush=True)
            del X, buf
        del Psi, fac, summ
        torch.cuda.empty_cache()
    return report


def univariate(kinds, fac, degree):
    """psi[v][k] as torch rows by the contract's recurrences (for the torch yardstick's Psi only)."""
    k = np.arange(13, dtype=np.float64)
    a, b, s = (2 * k + 1) / (k + 1), k / (k + 1), np.sqrt(2 * k + 1)
    h = 1.0 / np.sqrt(np.array([float(np.prod(np.arange(1, i + 1))) for i in range(13)]))
    out = []
    for v, kind in enumerate(kinds):
        x = fac[v] if kind == _abi.DESIGN_NORMAL else 2.0 * fac[v] - 1.0
        prev, cur = torch.ones_like(x), x
        psi = [torch.ones_like(x), (h[1] if kind == _abi.DESIGN_NORMAL else s[1]) * cur]
        for d in range(1, degree):
            nxt = (x * cur) - (float(d) * prev) if kind == _abi.DESIGN_NORMAL else ((a[d] * x) * cur) - (b[d] * prev)
            prev, cur = cur, nxt
            psi.append((h[d + 1] if kind == _abi.DESIGN_NORMAL else s[d + 1]) * cur)
        out.append(psi)
    return out


def flights(args):
    from erpl_monte_carlo_sim_amd import sampling
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    N = args.flights
    rows = [_abi.SUM_FIRST_APOGEE_ALT, _abi.SUM_RANGE]
    t0 = time.perf_counter()
    run = mc.run_monte_carlo_device(dict(EXAMPLE_IC), N, seed=1234, planar=True, design="lhs")
    t1 = time.perf_counter()
    sur = mc.surrogate(run, rows=rows, degree=2, order=2, holdout=5)
    t2 = time.perf_counter()
    every = sampling.scalar_primitives(100)
    five = ("mass", "motor_thrust", "motor_mass_flow", "wind_speed", "wind_direction")
    sob = mc.sobol_indices(dict(EXAMPLE_IC), n_base=N, groups={k: [every[k]] for k in five}, rows=rows, seed=1234, planar=True,
                           design="lhs")
    t3 = time.perf_counter()
    out = {"flights": N, "planar": True, "design": "lhs", "degree": 2, "order": 2, "holdout": 5, "n_terms": sur["n_terms"],
           "count": sur["count"], "n_fit": sur["n_fit"], "n_val": sur["n_val"], "variables": sur["names"], "fly_s": t1 - t0,
           "surrogate_s": t2 - t1, "sobol_flights": sob["performance"]["flights"], "sobol_s": t3 - t2, "rows": {}}
    for j, name in enumerate(sur["row_names"]):
        r = {"r2": float(sur["r2"][j]), "q2": float(sur["q2"][j]), "ranking": sur["ranking"][j][:6],
             "interactions": sur["interactions"][j][:5], "compare": {}}
        for g, key in enumerate(five):
            v = sur["names"].index(key)
            r["compare"][key] = {"pce_first": float(sur["first"][j][v]), "pce_total": float(sur["total"][j][v]),
                                 "pce_first_times_r2": float(sur["first"][j][v] * sur["r2"][j]),
                                 "pce_total_times_r2": float(sur["total"][j][v] * sur["r2"][j]),
                                 "sobol_first": [float(np.asarray(sob["first"][q])[j][g]) for q in ("lo", "estimate", "hi")],
                                 "sobol_total": [float(np.asarray(sob["total"][q])[j][g]) for q in ("lo", "estimate", "hi")]}
        out["rows"][name] = r
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--points", type=int, default=10 ** 7)
    ap.add_argument("--lstsq-max", type=float, default=5e10)
    ap.add_argument("--gram-ms", type=float, nargs=3, default=None, help="time of the Gram kernels of one call per shape, from a trace")
    ap.add_argument("--flights", type=int, default=0)
    ap.add_argument("--only-flights", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="one of the three shapes (0..2) instead of all")
    ap.add_argument("--native-only", action="store_true", help="the calls of erpl_mc_surrogate alone (for a kernel trace)")
    ap.add_argument("--lib", default=None, help="path of an experiment build of liberpl_mc.so to time instead of the product")
    ap.add_argument("--out", default="profiles/surrogate_native_vs_torch.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    if args.lib:      # an experiment build of the library (another tile size): never the product
        from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
        eng = TrajectoryEngine(dev, lib_path=args.lib)
    else:
        eng = shared_engine(dev)
    report = {"what": "warm wall milliseconds of the whole erpl_mc_surrogate call (median of --calls); HIP-event milliseconds of the "
                      "torch product and of predict; gram_flops = 2 * P (P + 1) / 2 * n_fit",
              "fp64_vector_peak_TFLOPs": PEAK_TFLOPS}
    if not args.only_flights:
        report["shapes"] = timing(args, eng, dev)
    if args.flights:
        report["flights"] = flights(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
