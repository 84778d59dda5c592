"""Shared by tests/test_tally_abi.py (host) and tests/test_gpu_tally.py (device): the specs, as the plain dicts of tally_ref
and as the library's struct, the fixed tables they are run on, and the comparison of a state with the restatement."""
import math

import numpy as np

from erpl_monte_carlo_sim_amd import analysis

import tally_ref as R

BOUNDS = (80000.0, 100.0, 200000.0, 600.0, 1200.0 ** 2 / (2 * 9.81) * 1.2)
APOGEE, RANGE, FLIGHT_TIME, IMPACT_X, IMPACT_Y, FINAL_VZ, MAX_SPEED = 0, 4, 5, 8, 9, 14, 15
SIZES = (1, 63, 64, 65, 257, 1025)          # samples per add
PERCENT = [0.0, 0.5, 5.0, 25.0, 50.0, 75.0, 99.9, 100.0]
ZONES = [np.array([[-300.0, -200.0], [400.0, -250.0], [250.0, 300.0], [-100.0, 150.0]]),
         np.array([[0.0, 0.0], [900.0, 100.0], [100.0, 700.0]])]


BIG_GRID = (IMPACT_X, IMPACT_Y, 256, 200, -800.0, 800.0, -700.0, 900.0)   # wider than the LDS tile of the kernel, impacts all over it


def spec_dict(k=5, bins=(1024, 50, 1, 7, 3), zones=True, grid=None):
    """Five rows: apogee on 1024 bins, range with values on its edges, flight time on ONE bin, max speed (the exactness row:
    centre 0, so d = x) and final vz (a constant: ties across ids)."""
    return {"bounds": BOUNDS, "rows": [APOGEE, RANGE, FLIGHT_TIME, MAX_SPEED, FINAL_VZ], "bins": list(bins),
            "lo": [0.0, 0.0, 0.0, -1000.0, -50.0], "hi": [3000.0, 2400.0, 550.0, 1000.0, 50.0],
            "centre": [1500.0, 1200.0, 275.0, 0.0, -7.0],
            "thresholds": [[2500.0, 2990.0], [0.0, 2400.0, 1e9], [], [-np.inf, 0.0, 1e299], [-7.25]],
            "k": k, "percent": list(PERCENT), "grid": grid or (IMPACT_X, IMPACT_Y, 16, 9, -800.0, 800.0, -700.0, 900.0),
            "zones": [z.copy() for z in ZONES] if zones else []}


def library_spec(d):
    return analysis.tally_spec(rows=d["rows"], ranges=list(zip(d["lo"], d["hi"])), bins=d["bins"], centres=d["centre"],
                               thresholds=d["thresholds"], k=d["k"], quantiles=[p / 100 for p in d["percent"]],
                               bounds=dict(zip(("max_apogee", "min_apogee", "max_range", "max_flight_time", "energy_apogee"),
                                               d["bounds"])),
                               grid_rows=d["grid"][:2], grid_bins=d["grid"][2:4], grid_ranges=(d["grid"][4:6], d["grid"][6:8]),
                               zones=d["zones"])


EXACT = [1e300, 1.0, -1e300, 2.0 ** -60, -1.0, 1e150, -1e150, 1e150, 3.0000000000000004e149, 2.0 ** -500, 3e-200, -2.5e-200,
         2.0 ** -1074, 2.0 ** -485, -(2.0 ** -485) * (1 + 2.0 ** -52), 0.1, 0.2, 0.30000000000000004, 1e-17, 123456.789,
         2.0 ** 500, -(2.0 ** 500), np.nextafter(2.0 ** 500, 0.0), 5e-324, -0.0, 0.0]


def table(n, seed=7, all_outliers=False):
    """summary [16, n], status [n]: finite bulk with what goes wrong mixed in."""
    rs = np.random.RandomState(seed)
    s = rs.uniform(-1.0, 1.0, (16, n))
    s[APOGEE] = rs.uniform(200.0, 2999.0, n)
    s[RANGE] = rs.randint(0, 51, n) * 48.0            # on the edges of 50 bins over 0..2400, 2400 = hi included
    s[FLIGHT_TIME] = rs.uniform(10.0, 540.0, n)
    s[FINAL_VZ] = -7.25                                # every value equal: ties that only the id breaks
    s[MAX_SPEED] = np.array(EXACT)[rs.randint(0, len(EXACT), n)] * rs.choice([1.0, 1.0, 1.0, 0.5, -2.0], n)
    s[IMPACT_X] = rs.normal(0.0, 350.0, n)
    s[IMPACT_Y] = rs.normal(50.0, 300.0, n)
    pick = lambda every, off: np.arange(off, n, every)
    s[IMPACT_Y, pick(11, 3)] = -200.0                  # level with a polygon vertex
    s[IMPACT_Y, pick(13, 5)] = 100.0
    s[IMPACT_X, pick(17, 2)] = 400.0
    s[IMPACT_X, pick(29, 7)] = -800.0                  # on the grid's border
    s[IMPACT_Y, pick(31, 9)] = 900.0
    s[IMPACT_X, pick(37, 1)] = 5000.0                  # off the grid
    s[IMPACT_Y, pick(41, 4)] = np.nan
    s[MAX_SPEED, pick(19, 6)] = np.nan
    s[MAX_SPEED, pick(23, 8)] = np.inf
    s[MAX_SPEED, pick(27, 10)] = -np.inf
    s[MAX_SPEED, pick(7, 0)] = -0.0
    s[MAX_SPEED, pick(9, 1)] = 0.0
    s[APOGEE, pick(16, 11)] = 3000.0                   # exactly hi
    s[APOGEE, pick(33, 12)] = 0.0 + 150.0              # in range, below most
    s[APOGEE, pick(43, 13)] = 50.0                     # apogee low: an outlier
    s[APOGEE, pick(47, 14)] = 90000.0                  # apogee high and energy
    s[APOGEE, pick(53, 15)] = np.nan
    s[RANGE, pick(59, 16)] = 250000.0
    s[FLIGHT_TIME, pick(61, 17)] = 601.0
    s[FLIGHT_TIME, pick(67, 18)] = np.inf
    s[FLIGHT_TIME, pick(21, 19)] = 549.9               # valid, below hi = 550
    s[FLIGHT_TIME, pick(45, 20)] = 575.0               # valid (<= 600), above hi = 550
    if all_outliers:
        s[APOGEE] = np.where(np.arange(n) % 2 == 0, 1e6, np.nan)
    status = (np.arange(n) % 5).astype(np.int32)
    status[pick(10, 3)] |= 1 << 10
    status[pick(6, 1)] |= 1 << 9
    return np.ascontiguousarray(s), status


def host_tally(spec, pieces):
    """The state after one erpl_mc_tally_add_host per (summary, status, first_id) of `pieces`."""
    state = np.zeros(analysis.tally_words(spec), dtype=np.int64)
    for summary, status, first_id in pieces:
        analysis.tally_add_host(spec, state, summary, status, first_id)
    return state


def check_against_ref(spec_d, spec, state, ref):
    """Everything a result holds against the restatement."""
    got = analysis.tally_result_host(spec, state)
    res = got["result"]
    assert (res.n, res.n_valid, res.n_outliers) == (ref["n"], ref["n_valid"], ref["n"] - ref["n_valid"])
    assert list(res.reason_counts) == ref["reason_counts"]
    assert list(res.termination_counts) == ref["termination_counts"]
    assert (res.n_status_nan, res.n_incomplete) == (ref["n_status_nan"], ref["n_incomplete"])
    k = spec_d["k"]
    for j, want in enumerate(ref["rows"]):
        row, bins = res.row[j], spec_d["bins"][j]
        assert (row.count, row.below, row.above, row.moment_skipped) == \
            (want["count"], want["below"], want["above"], want["moment_skipped"]), j
        assert list(row.exceed[:len(want["exceed"])]) == want["exceed"], j
        assert np.array_equal(got["hist_counts"][j, :bins], want["hist"]), j        # np.histogram on the counted values
        assert not got["hist_counts"][j, bins:].any()
        # the exact sums, to the bit
        assert row.sum_d == want["sum_d"] and math.copysign(1, row.sum_d) == math.copysign(1, want["sum_d"]), (j, row.sum_d, want["sum_d"])
        assert row.sum_d2 == want["sum_d2"], (j, row.sum_d2, want["sum_d2"])
        for name in ("mean", "var", "std"):
            a, b = getattr(row, name), want[name]
            assert a == b or (math.isnan(a) and math.isnan(b)), (j, name, a, b)
        small = [(row.smallest[e].value, row.smallest[e].id) for e in range(row.n_smallest)]
        large = [(row.largest[e].value, row.largest[e].id) for e in range(row.n_largest)]
        assert row.n_smallest == row.n_largest == min(k, want["count"]), j
        for mine, theirs in ((small, want["smallest"]), (large, want["largest"])):
            assert [i for _, i in mine] == [i for _, i in theirs], j
            assert [np.float64(v).view(np.uint64) for v, _ in mine] == [np.float64(v).view(np.uint64) for v, _ in theirs], j
        if k > 0 and want["count"] > 0:
            assert (row.min, row.max) == (want["smallest"][0][0], want["largest"][0][0])
        else:
            assert math.isnan(row.min) and math.isnan(row.max)
        check_quantiles(spec_d, j, row, want)
    assert (res.grid_counted, res.grid_outside) == (ref["grid_counted"], ref["grid_outside"])
    assert np.array_equal(got["grid_counts"], ref["cells"])                          # np.histogram2d on the counted values
    assert list(res.zone_inside[:len(ref["zone_inside"])]) == ref["zone_inside"]
    return got


def check_quantiles(spec_d, j, row, want):
    count, k = want["count"], spec_d["k"]
    width = (spec_d["hi"][j] - spec_d["lo"][j]) / spec_d["bins"][j]
    held = lambda r: r < min(k, count) or r >= count - min(k, count)
    in_range = lambda r: spec_d["lo"][j] <= want["sorted"][r] <= spec_d["hi"][j]
    for i, p in enumerate(spec_d["percent"]):
        got, exact = row.quantile[i], row.quantile_exact[i]
        if count == 0:
            assert math.isnan(got) and exact == 0
            continue
        r0, r1 = R.order_statistics(count, p / 100)
        truth = np.percentile(want["sorted"], p)
        if held(r0) and held(r1):
            assert exact == 1 and (got == truth or (math.isnan(got) and math.isnan(truth))), (j, p, got, truth)   # to the bit
        elif all(held(r) or in_range(r) for r in (r0, r1)):
            assert exact == 0 and abs(got - truth) <= width, (j, p, got, truth, width)
        else:   # an order statistic in the below / above mass that is not held
            assert exact == 0 and math.isnan(got), (j, p, got)
