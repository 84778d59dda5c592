#!/usr/bin/env python3
"""erpl_mc_corridor_drivers beside a torch fp64 restatement of the same sums in the same process and beside the NumPy
restatement tests/corridor_drivers_ref.py.

Warm (`--warmup` calls), median of `--calls` host-timed calls, every window closed by a device synchronise:

  call     (m, F, rows) = `--m`, `--factors`, `--rows` on synthetic data on the device (30 % NaN in the values, 10 % of the
           mask bytes set, one pair of factors correlated at 0.57), with and without the regression; the FMAs of the product
           pass as the kernel issues them (whole 16-column blocks) and as the definitions need them, and the bytes of `values`
  copy     `values` copied on the device (y.clone(): read + written), the rate the bytes of the product pass are held against
  torch    the same masked sums of standardised data by torch.where and `@` in fp64, `--torch-chunk` columns at a time
  numpy    the restatement on `--host-rows` rows, one process, EXTRAPOLATED to all rows (0: skipped)

`--lib PATH` loads another build of the library (an experiment build, never the product): the v_fma_f64 build of the product
pass (-DERPL_CDRV_MFMA=0).  `--calls-only` runs the calls alone, for a kernel trace of the passes."""
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


def torch_sums(x, y, mask, chunk):
    """The sums of the product pass, the regression's pairs included: returns (lin [2 R, F + 1], pairs [R, F (F + 1) / 2])."""
    F, m = x.shape
    R = y.shape[0]
    base = (mask == 0) & torch.isfinite(x).all(dim=0)
    xb = torch.where(base, x, torch.zeros((), dtype=x.dtype, device=x.device))
    nb = base.sum()
    xmean = xb.sum(dim=1) / nb
    xstd = torch.sqrt((torch.where(base, x - xmean[:, None], 0.0) ** 2).sum(dim=1) / nb)
    mem = base & torch.isfinite(y)
    cnt = mem.sum(dim=1)
    ymean = torch.where(mem, y, 0.0).sum(dim=1) / cnt
    ystd = torch.sqrt((torch.where(mem, y - ymean[:, None], 0.0) ** 2).sum(dim=1) / cnt)
    iu = torch.triu_indices(F, F, device=x.device)
    lin = torch.zeros((2 * R, F + 1), dtype=x.dtype, device=x.device)
    pairs = torch.zeros((R, iu.shape[1]), dtype=x.dtype, device=x.device)
    for a in range(0, m, chunk):
        b = min(m, a + chunk)
        xs = torch.where(base[a:b], (x[:, a:b] - xmean[:, None]) / xstd[:, None], 0.0)
        ys = torch.where(mem[:, a:b], (y[:, a:b] - ymean[:, None]) / ystd[:, None], 0.0)
        left = torch.cat([mem[:, a:b].to(x.dtype), ys], dim=0)
        right = torch.cat([xs, torch.ones((1, b - a), dtype=x.dtype, device=x.device)], dim=0)
        lin += left @ right.T
        pairs += left[:R] @ (xs[iu[0]] * xs[iu[1]]).T
    return lin, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--factors", type=int, default=19)
    ap.add_argument("--rows", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=65536)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    eng = TrajectoryEngine(torch.device("cuda", 0), lib_path=args.lib)
    dev, m, F, R = eng.device, args.m, args.factors, args.rows
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    x = torch.randn((F, m), dtype=torch.float64, device=dev, generator=g)
    if F > 1:
        x[1] = 0.57 * x[0] + (1.0 - 0.57 ** 2) ** 0.5 * x[1]
    x += 10.0 * torch.arange(F, dtype=torch.float64, device=dev)[:, None]
    coef = torch.randn((R, F), dtype=torch.float64, device=dev, generator=g)
    y = coef @ (x - x.mean(dim=1, keepdim=True)) + torch.randn((R, m), dtype=torch.float64, device=dev, generator=g)
    y.masked_fill_(torch.rand((R, m), device=dev, generator=g) < 0.3, float("nan"))
    mask = (torch.rand((m,), device=dev, generator=g) < 0.1).to(torch.uint8)
    del coef

    P = F * (F + 1) // 2
    blocks = lambda cols: 16 * ((cols + 15) // 16)
    res = {"label": args.label, "m": m, "factors": F, "rows": R, "values_bytes": 8 * R * m,
           "fma_defined": {"regression": R * m * (2 * F + 2 + P), "pearson_only": R * m * (3 * F + 2)},
           "fma_issued": {"regression": 32 * ((R + 31) // 32) * m * (2 * 48 + blocks(P)),
                          "pearson_only": 32 * ((R + 31) // 32) * m * (2 * 48 + blocks(F))}}
    box = {}

    def call(regression):
        box[regression] = eng.corridor_drivers(x, y, mask=mask, regression=regression)

    res["call_regression"] = wall(lambda: call(True), args.warmup, args.calls)
    res["call_pearson_only"] = wall(lambda: call(False), args.warmup, args.calls)
    out = box[True]
    # the device copy of `values` (read + written) in the same process: the rate the bytes of the product pass are held against
    res["copy_values"] = wall(lambda: box.__setitem__("copy", y.clone()), 1, args.calls)
    res["copy_values"]["bytes"] = 2 * 8 * R * m
    box.pop("copy")
    res["rows_ok"] = int(out["regression_ok"].sum())
    if not args.calls_only:
        res["torch"] = wall(lambda: box.__setitem__("torch", torch_sums(x, y, mask, args.torch_chunk)), 1, args.calls)
        # the torch sums give the device's correlations: the figure that says both computed the same thing
        lin, _ = box["torch"]
        lin = lin.cpu().numpy()
        n = lin[:R, F]
        with np.errstate(all="ignore"):
            sxy = lin[R:, :F] - lin[:R, :F] * (lin[R:, F] / n)[:, None]
        res["torch_sxy_finite"] = bool(np.isfinite(sxy[n > 1]).all())
        if args.host_rows > 0:
            import corridor_drivers_ref as ref
            hx, hy, hm = x.cpu().numpy(), y[:args.host_rows].cpu().numpy(), mask.cpu().numpy()
            t0 = time.perf_counter()
            want = ref.restate(hx, hy, hm)
            sec = time.perf_counter() - t0
            res["numpy"] = {"rows_timed": args.host_rows, "seconds": sec, "seconds_extrapolated_to_all_rows": sec / args.host_rows * R,
                            "max_abs_pearson_difference": float(np.nanmax(np.abs(out["pearson"][:args.host_rows] - want["pearson"]))),
                            "max_abs_src_difference": float(np.nanmax(np.abs(out["src"][:args.host_rows] - want["src"])))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
