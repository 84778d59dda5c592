#!/usr/bin/env python3
"""erpl_mc_corridor_bands_weighted beside erpl_mc_corridor_bands on the same (3, 256, m) matrix in the same process, and against
the NumPy restatement in one host process.  Writes profiles/corridor_w_bench.json.

Every GPU step runs in a child process of its own under its own time limit (`--limit` seconds); the first step that fails or
runs out of time ends the run.  Warm (`--warmup` calls), median of `--calls` host-timed calls, every window closed by a device
synchronise:

  synth M     (3, 256, M) for every `--m`: synthetic normal rows with 2 % NaN and 10 % masked columns (section 8.7's matrix),
              weights of an importance sampler - W = floor(2^Q exp(l - l_max)) for a normal log-ratio l - with 5 % zeros.
              Per step the weighted call, the unweighted call, their ratio, the bytes the ten passes of the weighted kernel
              read (values and weights, 16 bytes per column and pass) per second of the whole call, and the restatement
              (stable argsort on the key + cumulative weight per row, the moments) on `--host-rows` rows, EXTRAPOLATED
              linearly to all rows.
  trace M     the kernels of one weighted and one unweighted call at `--trace-m` columns from a `rocprofv3 --kernel-trace
              --stats` run of its own (a child process under the profiler); UNMEASURED where the profiler gives nothing.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = (0.05, 0.25, 0.5, 0.75, 0.95)
PASSES = 10   # moments, centred, eight digit passes


def wall(fn, warmup, calls):
    import torch
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


def synthetic(eng, m):
    import torch
    gen = torch.Generator(device=eng.device).manual_seed(7)
    x = torch.randn((3, 256, m), dtype=torch.float64, device=eng.device, generator=gen)
    x[torch.rand((3, 256, m), device=eng.device, generator=gen) < 0.02] = float("nan")
    mask = (torch.rand((m,), device=eng.device, generator=gen) < 0.1).to(torch.uint8)
    z = torch.randn((m,), dtype=torch.float64, device=eng.device, generator=gen)
    l = 0.5 * z - 0.125 * z * z                      # the log-ratio of N(0.4, 0.8^2) to N(0, 1), up to a constant
    q_bits = min(52, 62 - (m - 1).bit_length())
    w = torch.floor(torch.ldexp(torch.exp(l - l.max()), torch.tensor(q_bits, device=eng.device))).to(torch.int64)
    w[torch.rand((m,), device=eng.device, generator=gen) < 0.05] = 0
    return x, mask, w


def host_rows(rows, keep, w, qs):
    """The restatement's work on some rows."""
    t0 = time.perf_counter()
    for row in rows:
        use = keep & np.isfinite(row) & (w > 0)
        xs, ws = row[use], w[use]
        if not len(xs):
            continue
        b = xs.view(np.uint64)
        key = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
        order = np.argsort(key, kind="stable")
        cum = np.cumsum(ws[order].astype(np.uint64))
        S = int(cum[-1])
        for q in qs:
            t = min(max(int(np.ceil(q * float(S))), 1), S)
            xs[order][int(np.searchsorted(cum, np.uint64(t), side="left"))]
        wd = ws.astype(np.float64)
        mean = float(np.sum(wd * xs) / np.sum(wd))
        d = xs - mean
        np.sum(wd * d * d), np.sum(wd * wd * d * d), np.sum(wd * wd)
    return time.perf_counter() - t0


def step(args):
    import torch  # noqa: F401
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    eng = shared_engine(None)
    kind, _, size = args.step.partition(":")
    m = int(size)
    x, mask, w = synthetic(eng, m)
    weighted = lambda: eng.corridor_bands_weighted(x, w, mask=mask, quantiles=Q)   # noqa: E731
    flat = lambda: eng.corridor_bands(x, mask, quantiles=Q)                        # noqa: E731
    if kind == "trace":   # under the profiler: one warm call of each is all it needs
        for _ in range(2):
            weighted()
            flat()
        torch.cuda.synchronize()
        print("RESULT {}")
        return
    C, T = 3, 256
    res = {"shape": [C, T, m], "matrix_bytes": C * T * m * 8}
    res["weighted"] = wall(weighted, args.warmup, args.calls)
    res["unweighted"] = wall(flat, args.warmup, args.calls)
    res["ratio"] = res["weighted"]["median_ms"] / res["unweighted"]["median_ms"]
    res["weighted_bytes_read"] = PASSES * C * T * m * 16
    res["weighted_bytes_per_s"] = res["weighted_bytes_read"] / (1e-3 * res["weighted"]["median_ms"])
    res["unweighted_bytes_per_s"] = PASSES * C * T * m * 8 / (1e-3 * res["unweighted"]["median_ms"])
    rows = x.reshape(-1, m)[:: max(1, C * T // args.host_rows)][:args.host_rows].cpu().numpy()
    sec = host_rows(rows, (mask == 0).cpu().numpy(), w.cpu().numpy(), Q)
    res["numpy"] = {"rows_timed": len(rows), "rows_s": sec, "rows_s_EXTRAPOLATED": sec * C * T / len(rows)}
    print("RESULT " + json.dumps(res))


def trace(args):
    """The per-kernel statistics of a `rocprofv3 --kernel-trace --stats` run of the trace step."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--step", f"trace:{args.trace_m}"]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except (subprocess.TimeoutExpired, FileNotFoundError) as e:
            return f"UNMEASURED: {e!r}"
        if out.returncode != 0:
            return f"UNMEASURED: exit status {out.returncode}: {out.stderr[-300:]}"
        kernels = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    for kernel in ("bw_rows", "bw_scan_finish", "bw_scan", "erpl_corridor_bands"):
                        if kernel in name:   # (the first that matches: bw_scan_finish before bw_scan)
                            kernels[kernel] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]),
                                               "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"])}
                            break
        return {"m": args.trace_m, "kernels": kernels} if kernels else "UNMEASURED: the profiler wrote no kernel statistics"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="*", default=[8192, 131072, 1048576])
    ap.add_argument("--trace-m", type=int, default=131072)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=12)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a step may take")
    ap.add_argument("--step", default=None, help="internal: the step a child process runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corridor_w_bench.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    res = {"warmup": args.warmup, "calls": args.calls, "quantiles": list(Q)}
    ok = True
    for m in args.m:
        s = f"synth:{m}"
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s] + \
              [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("warmup", "calls", "host_rows")]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            res[s], ok = f"no result: over {args.limit} s", False
            break
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            res[s], ok = f"no result: exit status {out.returncode}: {out.stderr[-400:]}", False
            break
        res[s] = json.loads(line[-1][7:])
        print(f"# {s}: done", file=sys.stderr, flush=True)
    if ok:   # nothing more on the GPU behind a step that failed
        res["rocprofv3_kernel_trace"] = trace(args)
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
