#!/usr/bin/env python3
"""erpl_mc_correlation (TrajectoryEngine.correlation) against its torch equivalent on the same synthetic tensors, in ONE
process on the GPU: F = 19 factors (1 + 0.02 z, uniform and tied columns), R = 3 outcome rows that depend on them, a
mask that drops 5 % of the samples, at n = 10^6 and 10^7.

  native, ranks = 0     population + moments + Gram
  native, ranks = 1     the same + 22 x (keys, radix sort, rank scatter) + the Gram pass on the ranks
  torch corrcoef        torch.corrcoef on the stacked population (stacking and masking included, as the native call
                        includes them)
  torch ranks           per variable torch.sort + tie averaging (unique_consecutive) + scatter, then torch.corrcoef

Every figure is the median HIP-event time over `--calls` calls after `--warmup` warm-up calls; the native calls include the
host's wait for the result (they return when it is filled).  The Gram pass's bounds are reported beside it: it reads
(8 V + 1) n bytes and does V (V + 1) / 2 multiply-adds per sample (counted on the 4 x 4 blocks it really computes).

`--profile` runs three calls of each native form and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`
for the per-kernel split (population, moments, gram, keys, sort, rank scatter); `--kernel-stats FILE` folds the CSV of such
a run into the JSON."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from erpl_monte_carlo_sim_amd import _abi, flatten, models      # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine      # noqa: E402

HBM_ACHIEVABLE = 6.3e12     # bytes/s a streaming kernel reaches on the MI355X (tools/bench_analysis.py)
FP64_VECTOR_PEAK = 78.6e12  # flop/s of the fp64 vector pipes with FMA; without contraction (mul + add) half of it
ROWS = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
F = 19


def tensors(n, dev, seed=7):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    z = torch.randn((F, n), generator=g, dtype=torch.float64, device=dev)
    fac = torch.empty_like(z)
    fac[0::3] = 1.0 + 0.02 * z[0::3]
    fac[1::3] = 5.0 * torch.rand((len(range(1, F, 3)), n), generator=g, dtype=torch.float64, device=dev)
    fac[2::3] = torch.round(z[2::3] * 10.0) / 10.0
    summ = torch.randn((16, n), generator=g, dtype=torch.float64, device=dev)
    w = torch.randn((len(ROWS), F), generator=g, dtype=torch.float64, device=dev)
    summ[ROWS] = w @ (fac - fac.mean(dim=1, keepdim=True)) + 0.3 * summ[ROWS]
    mask = (torch.rand((n,), generator=g, device=dev) < 0.05).to(torch.uint8)
    return fac.contiguous(), summ.contiguous(), mask.contiguous()


def torch_population(fac, summ, mask):
    x = torch.cat([fac, summ[ROWS]])
    return x[:, (mask == 0) & torch.isfinite(x).all(dim=0)]


def torch_ranks(p):
    out = torch.empty_like(p)
    for v in range(p.shape[0]):
        vals, idx = torch.sort(p[v])
        _, inverse, counts = torch.unique_consecutive(vals, return_inverse=True, return_counts=True)
        first = torch.cumsum(counts, 0) - counts
        out[v, idx] = (first.to(torch.float64) + (counts.to(torch.float64) + 1.0) * 0.5)[inverse]
    return out


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=11)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default="profiles/correlation_native_vs_torch.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    eng = TrajectoryEngine(dev)
    eng.set_config(flatten.config_from_objects(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere()))
    V = F + len(ROWS)
    report = {"what": "median HIP-event milliseconds per call; synthetic tensors, F = 19, R = 3, 5 % masked",
              "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "fp64_vector_peak_flop_per_s": FP64_VECTOR_PEAK, "sizes": []}
    for n in args.sizes:
        fac, summ, mask = tensors(n, dev)
        native = {"native_pearson": lambda: eng.correlation(fac, summ, mask, rows=ROWS, ranks=False),
                  "native_with_ranks": lambda: eng.correlation(fac, summ, mask, rows=ROWS, ranks=True)}
        if args.profile:
            for fn in native.values():
                for _ in range(3):
                    fn()
            continue
        # the same answer first
        got = native["native_with_ranks"]()
        p = torch_population(fac, summ, mask)
        assert got["count"] == p.shape[1]
        assert float((torch.corrcoef(p).cpu() - torch.from_numpy(got["corr"])).abs().max()) < 1e-10
        assert float((torch.corrcoef(torch_ranks(p)).cpu() - torch.from_numpy(got["rank_corr"])).abs().max()) < 1e-10
        paths = dict(native)
        paths["torch_corrcoef"] = lambda: torch.corrcoef(torch_population(fac, summ, mask)).cpu()
        paths["torch_ranks_and_corrcoef"] = lambda: torch.corrcoef(torch_ranks(torch_population(fac, summ, mask))).cpu()
        row = {"n": n, "count": got["count"], "V": V}
        for k, fn in paths.items():
            row[k] = timed(fn, args.warmup, args.calls)
        nbk = (V + 3) // 4
        gram_bytes, gram_flop = (8 * V + 1) * n, 2 * 16 * (nbk * (nbk + 1) // 2) * n
        row["gram_pass_bytes"], row["gram_pass_flop"] = gram_bytes, gram_flop
        row["gram_pass_hbm_bound_ms"] = 1e3 * gram_bytes / HBM_ACHIEVABLE
        row["gram_pass_fp64_bound_ms"] = 1e3 * gram_flop / (FP64_VECTOR_PEAK / 2)
        row["torch_corrcoef_over_native_pearson"] = row["torch_corrcoef"]["median_ms"] / row["native_pearson"]["median_ms"]
        row["torch_ranks_over_native_with_ranks"] = (row["torch_ranks_and_corrcoef"]["median_ms"]
                                                     / row["native_with_ranks"]["median_ms"])
        report["sizes"].append(row)
        print(json.dumps(row), flush=True)
        del fac, summ, mask, p
        torch.cuda.empty_cache()
    if args.profile:
        return
    if args.kernel_stats:
        with open(args.kernel_stats) as fh:
            report["kernel_stats"] = [r for r in csv.DictReader(fh)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
