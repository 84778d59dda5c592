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
passes read 2 * 9 * n and the eight selection passes 8 * 9 * n."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--tile", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.6)
    ap.add_argument("--out", default="profiles/analysis_native_vs_torch.json")
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
    for tile in (1, args.tile):
        s = summ.repeat(1, tile).contiguous() if tile > 1 else summ
        t = status.repeat(tile).contiguous() if tile > 1 else status
        n = int(s.shape[1])
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


if __name__ == "__main__":
    main()
