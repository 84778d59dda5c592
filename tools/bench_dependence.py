#!/usr/bin/env python3
"""erpl_mc_dependence (TrajectoryEngine.dependence) against the same computation in NumPy, on one synthetic run per size
(m, F, R, M, H, P): outcomes that depend on the factors in a non-monotone way, nothing masked.

  native            HIP-event time of the call on its stream, warm (the call returns when the result is filled): median of
                    `--calls` after `--warmup` warm-up calls
  null share        the same with shifts = 0 (population, select, classes, class statistics, the F R tables of the run itself)
                    taken off: what the P F R null tables cost, as a share of the call
  table updates     P F R m pairs of class bytes over that time; every update reads one class byte and one cell byte, set
                    beside the streaming rates of MI355X_MICROARCH.md (the class bytes of a call fit the Infinity Cache
                    and, for the smaller size, an XCD's L2)
  conflicts         one factor and one row of m members, P null tables, twice: members in random order (an independent
                    pairing: the 64 lanes of a wave spread over the table) and x = y ascending in sample order (every wave's
                    1024 consecutive members share one class and one or two cells at any shift: the worst case of LDS
                    atomic conflicts).  The ratio is what cell conflicts cost.
  numpy             one process on the host: ranks and classes once per variable, then per table np.bincount and the
                    measures; timed on `--numpy-tables` tables and EXTRAPOLATED linearly to (1 + P) F R (said so in the report)
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

from erpl_monte_carlo_sim_amd import _abi, flatten, models      # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine              # noqa: E402

ALL_ROWS = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, _abi.SUM_MAX_SPEED]
HBM_TBS, MALL_TBS, L2_TBS = 6.29, 8.6, (16.8, 18.8)   # measured HBM copy rate; reads served by the Infinity Cache, by an XCD's L2


def synthetic(m, F, R, seed=7):
    rng = np.random.default_rng(seed)
    fac = rng.normal(size=(F, m))
    ys = np.empty((R, m))
    for j in range(R):
        ys[j] = 5.0 + np.sin(2.0 * fac[j % F]) + 0.5 * fac[(j + 1) % F] ** 2 + 0.3 * rng.normal(size=m)
    return fac, ys


def classes_of(x, K):
    """Mid-rank classes in NumPy (continuous data: no ties to average)."""
    order = np.argsort(x, kind="stable")
    rank = np.empty(len(x), dtype=np.int64)
    rank[order] = np.arange(1, len(x) + 1)
    return ((2 * rank - 1) * K) // (2 * len(x))


def measures(xc, yc, M, H):
    T = np.bincount(xc * H + yc, minlength=M * H).reshape(M, H).astype(np.int64)
    m = len(xc)
    n_c, col = T.sum(axis=1), T.sum(axis=0)
    delta = float(np.abs(m * T - np.outer(n_c, col)).sum()) / (2.0 * m * m)
    D = np.abs(m * np.cumsum(T, axis=1) - n_c[:, None] * np.cumsum(col)[None, :]).max(axis=1)
    ks = D[n_c > 0] / (float(m) * n_c[n_c > 0])
    cs, hs = np.nonzero(T)
    t = T[cs, hs].astype(np.float64)
    mi = float(((t / m) * np.log((t * m) / (n_c[cs] * col[hs].astype(np.float64)))).sum())
    return delta, float(ks.max()), float(np.median(ks)), mi


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
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 19, 3, 16, 16, 200, 1048576, 32, 4, 32, 32, 1000],
                    help="m F R M H P sextuples")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--numpy-tables", type=int, default=20)
    ap.add_argument("--out", default="profiles/dependence_native_vs_numpy.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = TrajectoryEngine(dev)
    eng.set_config(flatten.config_from_objects(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere()))
    report = {"what": "HIP-event milliseconds per call of TrajectoryEngine.dependence, warm; null share = (call - call with "
                      "shifts = 0) / call; table updates = P F R m over that difference, two class bytes read per update; "
                      "conflicts: F = R = 1, members in random order against x = y ascending in sample order; numpy: one "
                      "host process, timed on numpy_tables tables and extrapolated linearly to (1 + P) F R",
              "guide_TB_per_s": {"hbm": HBM_TBS, "infinity_cache": MALL_TBS, "l2_resident": list(L2_TBS)}, "sizes": []}
    s = args.sizes
    for m, F, R, M, H, P in zip(s[0::6], s[1::6], s[2::6], s[3::6], s[4::6], s[5::6]):
        fac, ys = synthetic(m, F, R)
        rows = ALL_ROWS[:R]
        d_summ = torch.zeros((_abi.SUMMARY_DIM, m), dtype=torch.float64, device=dev)
        for j, r in enumerate(rows):
            d_summ[r] = torch.from_numpy(ys[j]).to(dev)
        d_fac = torch.from_numpy(fac).to(dev)

        def native(p=P, f=d_fac, summ=d_summ, rws=rows, null=False):
            return eng.dependence(f, summ, rows=rws, classes=M, cells=H, shifts=p, seed=11, want_curves=False, want_null=null)

        # the same numbers first: the first numpy_tables null tables of pair (0, 0)
        nt = min(args.numpy_tables, P)
        got = native(nt, null=True)
        assert got["count"] == m
        t0 = time.perf_counter()
        xc, yc = classes_of(fac[0], M), classes_of(ys[0], H)
        class_s = time.perf_counter() - t0
        shifts = []
        lib = _abi.load_library()
        one = np.empty(1, dtype=np.int64)
        for p in range(nt):
            _abi.check(lib, lib.erpl_mc_bootstrap_indices(11, 0, m - 1, p, 1, one.ctypes.data), "erpl_mc_bootstrap_indices")
            shifts.append(int(one[0]) + 1)
        t0 = time.perf_counter()
        ref = np.array([measures(xc, np.roll(yc, -sh), M, H) for sh in shifts]).T
        table_s = (time.perf_counter() - t0) / max(nt, 1)
        err = float(np.max(np.abs(got["null_values"][0, 0] - ref)))
        assert err < 1e-12, err
        full, bare = event_ms(native, args.warmup, args.calls), event_ms(lambda: native(0), args.warmup, args.calls)
        null_ms = full["median_ms"] - bare["median_ms"]
        updates = P * F * R * m
        row = {"m": m, "F": F, "R": R, "M": M, "H": H, "P": P, "tables": (1 + P) * F * R, "native": full,
               "native_without_shifts": bare, "null_tables_ms": null_ms, "null_share": null_ms / full["median_ms"],
               "table_updates": updates, "table_updates_per_s": updates / (1e-3 * null_ms),
               "class_bytes_read_TB_per_s": 2 * updates / (1e-3 * null_ms) / 1e12, "class_bytes_of_the_call": (F + 2 * R) * m,
               "numpy_tables_timed": nt, "numpy_ms_per_table": 1e3 * table_s, "numpy_ms_classes_per_variable": 1e3 * class_s / 2,
               "numpy_ms_extrapolated": 1e3 * (table_s * (1 + P) * F * R + class_s / 2 * (F + R)), "max_abs_difference": err}
        row["numpy_over_native"] = row["numpy_ms_extrapolated"] / full["median_ms"]
        # what cell conflicts cost: one pair, members in random order against members in ascending order
        conflict = {}
        for name, x in (("independent", fac[0]), ("ascending", np.arange(m, dtype=np.float64))):
            one_summ = torch.zeros((_abi.SUMMARY_DIM, m), dtype=torch.float64, device=dev)
            one_summ[rows[0]] = torch.from_numpy(ys[0] if name == "independent" else x).to(dev)
            one_fac = torch.from_numpy(x[None, :].copy()).to(dev)
            t_full = event_ms(lambda: native(P, one_fac, one_summ, rows[:1]), args.warmup, args.calls)
            t_bare = event_ms(lambda: native(0, one_fac, one_summ, rows[:1]), args.warmup, args.calls)
            ms = t_full["median_ms"] - t_bare["median_ms"]
            conflict[name] = {"null_tables_ms": ms, "table_updates_per_s": P * m / (1e-3 * ms)}
            del one_summ, one_fac
        conflict["ascending_over_independent"] = conflict["ascending"]["null_tables_ms"] / conflict["independent"]["null_tables_ms"]
        row["conflicts"] = conflict
        report["sizes"].append(row)
        print(json.dumps(row), flush=True)
        del d_summ, d_fac
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
