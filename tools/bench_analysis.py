#!/usr/bin/env python3
"""analysis.native_statistics (erpl_mc_analyze: streaming passes + radix selection) against analysis.device_statistics
(torch ops, three full sorts) on the summary and status of a real f64_fast run of Set S, in ONE process on the GPU.

n samples are integrated once; the same tensors tiled `--tile` times give the larger size.  Both paths are warmed up,
then alternated for `--rounds` rounds; every timed window repeats one path until `--window` seconds have passed and is
closed by a device synchronise.  Writes medians and min-max spread of both paths at both sizes, and the native path's
algorithmic bytes per second and its share of the HBM rate (a whole-call figure: launches and the host's wait included,
not a kernel's share of peak), as JSON.

Algorithmic traffic of the native path (what the passes must read and write, not what a profiler counts): classify
reads (3 * 8 + 4) * n bytes and writes 2 n (the workspace bytes and the caller's copy); per described row the two moment
passes read 2 * 9 * n and the eight selection passes 8 * 9 * n.

`--distributions` adds, on the same tensors and the reason bytes of erpl_mc_analyze: erpl_mc_histogram (the three default
rows, 50 bins; range from the data = range pass + bin pass, and with explicit ranges = the bin pass alone: 9 n bytes per
row and pass), erpl_mc_histogram_xy (200 x 200, range from the data) and erpl_mc_dispersion, beside torch.histc on the
masked device columns and np.histogram on host copies of them; written to `--dist-out`."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from erpl_monte_carlo_sim_amd import _abi, analysis, flatten, models, sampling   # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine                      # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12   # bytes/s: the MI355X's HBM3E peak, and what a streaming kernel reaches of it
EXAMPLE_IC = {"position": [0.0, 0.0, 10.0], "velocity": [0, 0, 0.0], "attitude": [0.0, -1.5507963267948966, 0.0],
              "angular_velocity": [0.0, 0.0, 0.0]}


def native_bytes(n, n_rows=3, select_passes=8):
    return (3 * 8 + 4) * n + 2 * n + n_rows * (2 * 9 * n + select_passes * 9 * n)


def window(fn, seconds):
    """Calls per second of fn over a window of at least `seconds`, closed by a device synchronise."""
    torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while True:
        fn()
        calls += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def distribution_legs(eng, s, t, n, args):
    """The histogram / dispersion calls on the tensors of one size, beside torch.histc and np.histogram."""
    import numpy as np
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
    _, why = eng.analyze(s, t, rows=[], quantiles=[], reasons=True)
    valid = why == 0
    edges, counts, info = eng.histogram(s, why, rows=rows, bins=50)
    ranges = [(float(e[0]), float(e[-1])) for e in edges]
    cols = [s[r][valid] for r in rows]
    host_cols = [c.cpu().numpy() for c in cols]
    for j, c in enumerate(host_cols):                      # the same answer first
        ref_counts, ref_edges = np.histogram(c, 50)
        assert np.array_equal(ref_counts, counts[j]) and np.array_equal(ref_edges, edges[j]), rows[j]

    def torch_histc():   # masking included, as the native call includes it; one host read so that the call is complete
        out = [torch.histc(s[r][valid], bins=50) for r in rows]
        return out[-1][0].item()

    paths = {"native_histogram_auto_range": lambda: eng.histogram(s, why, rows=rows, bins=50),
             "native_histogram_explicit_range": lambda: eng.histogram(s, why, rows=rows, bins=50, ranges=ranges),
             "torch_histc_masked": torch_histc,
             "numpy_histogram_host_columns": lambda: [np.histogram(c, 50) for c in host_cols],
             "native_histogram2d_200x200": lambda: eng.histogram2d(s, why, rows[0], rows[1], bins=200),
             "native_dispersion": lambda: eng.dispersion(s, why)}
    for fn in paths.values():
        fn()
        fn()
    times = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, fn in paths.items():
            times[k].append(window(fn, args.window))
    row = {"n": n, "n_valid": int(info["counted"][0])}
    for k, v in times.items():
        row[k] = {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v)}
    one_pass = len(rows) * 9 * n                           # 8 bytes of the row + 1 mask byte per sample and row
    row["bin_pass_algorithmic_bytes"] = one_pass
    row["bin_pass_bytes_per_s"] = one_pass / row["native_histogram_explicit_range"]["median_s"]
    row["auto_range_bytes_per_s"] = 2 * one_pass / row["native_histogram_auto_range"]["median_s"]
    row["bin_pass_share_of_achievable_hbm"] = row["bin_pass_bytes_per_s"] / HBM_ACHIEVABLE
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--tile", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.6)
    ap.add_argument("--out", default="profiles/analysis_native_vs_torch.json")
    ap.add_argument("--distributions", action="store_true", help="time the histogram / dispersion calls as well")
    ap.add_argument("--dist-out", default="profiles/distributions_native_vs_numpy.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda", 0)
    rocket, motor, atm, wm = models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel()
    eng = TrajectoryEngine(dev)
    eng.set_config(flatten.config_from_objects(rocket, motor, atm))
    db = sampling.synthetic_dispersions(args.n, rocket, motor, wm, EXAMPLE_IC, dev, precision=_abi.PREC_F64_FAST, seed=1234,
                                        engine=eng)
    summ, status = eng.run(db)
    torch.cuda.synchronize()
    del db
    report = {"what": "seconds per call, whole call incl. the host's wait for the result; Set S f64_fast summary + status",
              "rounds": args.rounds, "window_s": args.window, "hbm_peak_bytes_per_s": HBM_PEAK,
              "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "sizes": []}
    dist_report = {"what": "seconds per call, whole call incl. the host's wait for the result; Set S f64_fast summary, mask = "
                           "the reason bytes of erpl_mc_analyze; rows apogee / range / flight time, 50 bins",
                   "rounds": args.rounds, "window_s": args.window, "hbm_peak_bytes_per_s": HBM_PEAK,
                   "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "sizes": []}
    for tile in (1, args.tile):
        s = summ.repeat(1, tile).contiguous() if tile > 1 else summ
        t = status.repeat(tile).contiguous() if tile > 1 else status
        n = int(s.shape[1])
        if args.distributions:
            dist_report["sizes"].append(distribution_legs(eng, s, t, n, args))
        paths = {"torch": lambda: analysis.device_statistics(s, t),
                 "native": lambda: analysis.native_statistics(s, t, engine=eng)}
        ref, got = paths["torch"](), paths["native"]()          # warm-up of both, and the same answer
        assert got["n_samples"] == ref["n_samples"] and torch.equal(got["valid_mask"], ref["valid_mask"])
        for key in ("apogee_altitude", "range", "flight_time"):
            assert got[key]["min"] == ref[key]["min"] and got[key]["max"] == ref[key]["max"], key
        for _ in range(2):
            for fn in paths.values():
                fn()
        times = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():
                times[k].append(window(fn, args.window))
        row = {"n": n, "n_valid": got["n_samples"], "reason_counts": got["reason_counts"]}
        for k, v in times.items():
            row[k] = {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v)}
        nb = native_bytes(n)
        row["native_algorithmic_bytes"] = nb
        row["native_bytes_per_s"] = nb / row["native"]["median_s"]
        row["native_share_of_hbm_peak"] = row["native_bytes_per_s"] / HBM_PEAK
        row["native_share_of_achievable_hbm"] = row["native_bytes_per_s"] / HBM_ACHIEVABLE
        row["torch_over_native"] = row["torch"]["median_s"] / row["native"]["median_s"]
        report["sizes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("written", args.out)
    if args.distributions:
        with open(args.dist_out, "w") as fh:
            json.dump(dist_report, fh, indent=1)
        print("written", args.dist_out)


if __name__ == "__main__":
    main()
