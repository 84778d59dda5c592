#!/usr/bin/env python3
"""Reduce a rocprofv3 --kernel-trace of bench.py to what the hand-over sweep of the fp64 throughput build costs the stream
it runs on: per timed pass, how long the sweep dispatch (erpl_flight_f64 behind the erpl_flight_f64f launches) lasts, which
instantiation ran (registers, scratch), and how long after the sweep's START the next rail kernel of the same stream
starts - with one stream per lane (four hardware queues) that is the time the lane's next batch is held back.

    tools/sweep_gaps.py <dir with *kernel_trace.csv> <out.json> [warmup passes to skip]

Streams are told apart by the trace's Stream_Id column where it has one, by Queue_Id otherwise.

`lane_cycles` splits every stream's dispatches into batches (one per rail kernel) and reports, for the batches that carry
the whole sequence rail, main launch, adoption sweeps, hand-over sweep on ONE stream (one stream per lane), the duration
of each launch, the tail (end of the main launch to end of the hand-over sweep), the gap to the lane's next rail kernel
and the lane cycle (rail start to next rail start).  A kernel trace has one interval per dispatch: when the last working
wave of a dispatch ended is not in it.

`lanes` is the same split for every stream that carries rail kernels, wherever the sweeps of its batches ran (a lane
with a sweep stream has them elsewhere): main launch, end of the main launch to the start of the lane's next rail kernel,
and the lane cycle."""
import csv
import glob
import json
import os
import statistics
import sys


def load(dirname):
    rows = []
    for f in glob.glob(os.path.join(dirname, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            key = r.get("Stream_Id") if r.get("Stream_Id") not in (None, "", "0") else r.get("Queue_Id")
            rows.append({"s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]), "name": r["Kernel_Name"], "key": key,
                         "vgpr": int(r.get("VGPR_Count") or r.get("Arch_VGPR_Count") or 0), "scratch": int(r.get("Scratch_Size") or 0),
                         "grid": int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)})
    rows.sort(key=lambda r: r["s"])
    return rows


def is_sweep(name):
    i = name.find("erpl_flight_f64")
    return i >= 0 and not name[i + len("erpl_flight_f64"):].startswith("f")


def stats(xs):
    xs = sorted(xs)
    if not xs:
        return None
    return {"n": len(xs), "min": xs[0], "median": statistics.median(xs), "mean": sum(xs) / len(xs), "max": xs[-1]}


def main():
    d, out_path = sys.argv[1:3]
    skip = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rows = load(d)
    rails = [r for r in rows if "erpl_rail_f64f" in r["name"]]
    if len(rails) <= skip:
        raise SystemExit("only %d erpl_rail_f64f dispatches" % len(rails))
    t0 = rails[skip]["s"]
    # the headline leg: up to the first rail kernel of another build
    others = [r["s"] for r in rows if "erpl_rail_" in r["name"] and "erpl_rail_f64f" not in r["name"] and r["s"] > t0]
    t1 = min(others) if others else rows[-1]["e"] + 1
    leg = [r for r in rows if t0 <= r["s"] < t1]
    by_key = {}
    for r in leg:
        by_key.setdefault(r["key"], []).append(r)
    dur, gap_start, gap_end, shared = [], [], [], 0
    for key, rs in by_key.items():
        for i, r in enumerate(rs):
            if not is_sweep(r["name"]):
                continue
            dur.append((r["e"] - r["s"]) / 1e6)
            nxt = next((q for q in rs[i + 1:] if "erpl_rail_f64f" in q["name"]), None)
            if nxt is not None:
                gap_start.append((nxt["s"] - r["s"]) / 1e6)
                gap_end.append((nxt["s"] - r["e"]) / 1e6)
        shared += any(is_sweep(r["name"]) for r in rs) and any("erpl_rail_f64f" in r["name"] for r in rs)
    sweeps = [r for r in leg if is_sweep(r["name"])]
    cyc = {k: [] for k in ("rail_ms", "main_ms", "adoption_sweep_1_ms", "adoption_sweep_2_ms", "handover_sweep_ms", "tail_ms",
                           "handover_end_to_next_rail_start_ms", "lane_cycle_ms")}
    grids = set()
    for key, rs in by_key.items():
        starts = [i for i, r in enumerate(rs) if "erpl_rail_f64f" in r["name"]]
        for a, b in zip(starts, starts[1:] + [len(rs)]):
            batch = [r for r in rs[a:b] if "erpl_flight_" in r["name"] or "erpl_rail_" in r["name"]]
            fl = [r for r in batch[1:] if not is_sweep(r["name"])]
            ho = [r for r in batch[1:] if is_sweep(r["name"])]
            if len(ho) != 1 or not fl:
                continue            # the sweeps of this batch ran on another stream
            ms = lambda r: (r["e"] - r["s"]) / 1e6
            cyc["rail_ms"].append(ms(batch[0]))
            cyc["main_ms"].append(ms(fl[0]))
            for j, name in ((1, "adoption_sweep_1_ms"), (2, "adoption_sweep_2_ms")):
                if len(fl) > j:
                    cyc[name].append(ms(fl[j]))
            cyc["handover_sweep_ms"].append(ms(ho[0]))
            cyc["tail_ms"].append((ho[0]["e"] - fl[0]["e"]) / 1e6)
            grids.add(ho[0]["grid"])
            if b < len(rs):
                cyc["handover_end_to_next_rail_start_ms"].append((rs[b]["s"] - ho[0]["e"]) / 1e6)
                cyc["lane_cycle_ms"].append((rs[b]["s"] - batch[0]["s"]) / 1e6)
    lanes = {k: [] for k in ("main_ms", "main_end_to_next_rail_start_ms", "lane_cycle_ms")}
    for key, rs in by_key.items():
        starts = [i for i, r in enumerate(rs) if "erpl_rail_f64f" in r["name"]]
        for a, b in zip(starts, starts[1:]):
            main = next((r for r in rs[a + 1:b] if "erpl_flight_" in r["name"] and not is_sweep(r["name"])), None)
            if main is None:
                continue
            lanes["main_ms"].append((main["e"] - main["s"]) / 1e6)
            lanes["main_end_to_next_rail_start_ms"].append((rs[b]["s"] - main["e"]) / 1e6)
            lanes["lane_cycle_ms"].append((rs[b]["s"] - rs[a]["s"]) / 1e6)
    out = {"streams_with_dispatches": len(by_key), "streams_carrying_both_rail_and_sweep": int(shared),
           "sweep_registers": sorted({r["vgpr"] for r in sweeps}), "sweep_scratch_bytes": sorted({r["scratch"] for r in sweeps}),
           "sweep_dispatch_ms": stats(dur),
           "sweep_start_to_next_rail_start_on_its_stream_ms": stats(gap_start),
           "sweep_end_to_next_rail_start_on_its_stream_ms": stats(gap_end),
           "lane_cycles": dict({k: stats(v) for k, v in cyc.items()}, handover_sweep_grid_threads=sorted(grids)),
           "lanes": {k: stats(v) for k, v in lanes.items()},
           "note": "timed passes of the f64_fast leg only (the first %d passes are warm-up); a sweep on a stream of its own has its "
                   "next rail kernel two batches later or none at all" % skip}
    json.dump(out, open(out_path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
