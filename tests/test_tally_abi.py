"""erpl_mc_tally_* at the C boundary, as far as it goes without a GPU: struct layout against gcc, the new names, the exact
defaults, every refusal (before any device work, in the order the header lists, the context last: a NULL context and dummy
pointers show them all), the host check program, and erpl_mc_tally_add_host / _merge_host / _result_host against the tests'
own restatement of the contract (tally_ref): counts, exact sums, extremes, quantiles, bins, grid and zones, and the bytes of
the state under every split, order and merge tree."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

import tally_cases as TC
import tally_ref as R
from tally_cases import check_against_ref, host_tally

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
DUMMY = H.DUMMY


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


# ------------------------------------------------------------------------------------------------ the boundary
def test_struct_layout_matches_the_c_compiler(tmp_path):
    H.check_struct_layouts(tmp_path, (("erpl_tally_spec", "ErplTallySpec"), ("erpl_tally_extreme", "ErplTallyExtreme"),
                                      ("erpl_tally_row", "ErplTallyRow"), ("erpl_tally", "ErplTally")),
                           (("ERPL_TALLY_MAX_ROWS", _abi.TALLY_MAX_ROWS), ("ERPL_TALLY_MAX_BINS", _abi.TALLY_MAX_BINS),
                            ("ERPL_TALLY_MAX_THRESHOLDS", _abi.TALLY_MAX_THRESHOLDS), ("ERPL_TALLY_MAX_K", _abi.TALLY_MAX_K),
                            ("ERPL_TALLY_MAX_Q", _abi.TALLY_MAX_Q), ("ERPL_TALLY_MAX_GRID", _abi.TALLY_MAX_GRID),
                            ("ERPL_TALLY_MAX_ZONES", _abi.TALLY_MAX_ZONES), ("ERPL_TALLY_MAX_VERTICES", _abi.TALLY_MAX_VERTICES)))
    assert (_abi.TALLY_MAX_ROWS, _abi.TALLY_MAX_BINS, _abi.TALLY_MAX_K, _abi.TALLY_MAX_GRID) == (8, 1024, 64, 256)


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_tally_defaults", "erpl_mc_tally_words", "erpl_mc_tally_add", "erpl_mc_tally_merge", "erpl_mc_tally_result",
                 "erpl_mc_tally_add_host", "erpl_mc_tally_merge_host", "erpl_mc_tally_result_host"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)
    assert _abi.ABI_VERSION == 4


def test_defaults_are_exact(lib):
    spec = _abi.ErplTallySpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_tally_defaults(C.byref(spec)) == 0
    ana = _abi.ErplAnalysisSpec()
    assert lib.erpl_mc_analysis_defaults(C.byref(ana)) == 0
    for name in ("max_apogee", "min_apogee", "max_range", "max_flight_time", "energy_apogee"):
        assert getattr(spec, name) == getattr(ana, name)
    assert spec.n_rows == 3 and list(spec.rows) == [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, 0, 0, 0, 0, 0]
    assert list(spec.bins) == [1000, 1000, 1000, 0, 0, 0, 0, 0] and list(spec.n_thresholds) == [0] * 8
    assert list(spec.lo) == [0.0] * 8 and list(spec.hi) == [80000.0, 200000.0, 600.0, 0, 0, 0, 0, 0]
    assert list(spec.centre) == [40000.0, 100000.0, 300.0, 0, 0, 0, 0, 0]
    assert spec.k == 16 and spec.n_q == 5 and list(spec.q) == [0.05, 0.25, 0.5, 0.75, 0.95, 0, 0, 0]
    assert (spec.row_x, spec.row_y, spec.bins_x, spec.bins_y) == (_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y, 128, 128)
    assert (spec.lo_x, spec.hi_x, spec.lo_y, spec.hi_y) == (-200000.0, 200000.0, -200000.0, 200000.0)
    assert spec.n_zones == 0 and not any(spec.zone_first) and not any(spec.zone_x) and not any(spec.zone_y)
    assert not any(v for line in spec.threshold for v in line)
    assert lib.erpl_mc_tally_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()
    # 16 header words; per row 12 counts, 1000 bins, 2 x 70 accumulator words, 2 + 4 k of extremes; 10 + 128 x 128 of the grid
    assert analysis.tally_words(spec) == 16 + 3 * (12 + 1000 + 140 + 2 + 64) + 10 + 128 * 128


ENTRIES = ("words", "add", "add_host", "merge", "merge_host", "result", "result_host")


def call_entry(lib, entry, spec, state=DUMMY, other=DUMMY, summary=DUMMY, ld=8, n=8, first_id=0, result=None):
    sp = C.byref(spec) if spec is not None else None
    res = _abi.ErplTally()
    rp = C.byref(res) if result is None else None
    words = C.c_int64()
    rc = {"words": lambda: lib.erpl_mc_tally_words(sp, C.byref(words)),
          "add": lambda: lib.erpl_mc_tally_add(None, sp, state, summary, ld, None, n, first_id, None),
          "add_host": lambda: lib.erpl_mc_tally_add_host(sp, state, summary, ld, None, n, first_id),
          "merge": lambda: lib.erpl_mc_tally_merge(None, sp, state, other, None),
          "merge_host": lambda: lib.erpl_mc_tally_merge_host(sp, state, other),
          "result": lambda: lib.erpl_mc_tally_result(None, sp, state, rp, None, None, None),
          "result_host": lambda: lib.erpl_mc_tally_result_host(sp, state, rp, None, None)}[entry]()
    return rc, lib.erpl_mc_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_come_before_any_device_work_in_the_documented_order(lib, entry):
    def broken(upto):
        """A spec in which every check from number `upto` on fails: the earliest one has to be the one reported."""
        s = TC.library_spec(TC.spec_dict())
        bad = [lambda: setattr(s, "energy_apogee", math.nan),              # 0 a NaN bound
               lambda: setattr(s, "n_rows", 9),                           # 1 n_rows
               lambda: s.rows.__setitem__(1, 16),                         # 2 a row outside 0..15
               lambda: s.rows.__setitem__(3, s.rows[2]),                  # 3 a row listed twice
               lambda: s.bins.__setitem__(0, 1025),                       # 4 bins
               lambda: s.hi.__setitem__(0, s.lo[0]),                      # 5 an empty range
               lambda: s.centre.__setitem__(0, math.inf),                 # 6 centre
               lambda: s.n_thresholds.__setitem__(0, 9),                  # 7 n_thresholds
               lambda: s.threshold[1].__setitem__(0, math.nan),           # 8 a NaN threshold
               lambda: setattr(s, "k", 65),                               # 9 k
               lambda: setattr(s, "n_q", 9),                              # 10 n_q
               lambda: s.q.__setitem__(1, 1.5),                           # 11 q
               lambda: setattr(s, "row_x", -1),                           # 12 row_x
               lambda: setattr(s, "row_y", 16),                           # 13 row_y
               lambda: setattr(s, "bins_x", 0),                           # 14 bins_x  (row_x == row_y is shown on its own)
               lambda: setattr(s, "bins_y", 257),                         # 15 bins_y
               lambda: setattr(s, "hi_x", math.inf),                      # 16 range x
               lambda: setattr(s, "lo_y", math.nan),                      # 17 range y
               lambda: setattr(s, "n_zones", 9),                          # 18 n_zones
               ]
        for i in range(upto, len(bad)):
            bad[i]()
        return s

    rc, msg = call_entry(lib, entry, None)
    assert rc == -1 and "spec is NULL" in msg
    words = ["energy_apogee", "n_rows", "rows[1]", "rows[3]", "bins[0]", "lo[0]", "centre[0]", "n_thresholds[0]", "threshold[1]",
             "spec->k", "n_q", "q[1]", "row_x", "row_y", "bins_x", "bins_y", "lo_x", "lo_y", "n_zones"]
    for i, word in enumerate(words):
        rc, msg = call_entry(lib, entry, broken(i), state=None, other=None, summary=None, ld=-1, n=0, first_id=-1, result=None)
        assert rc == -1 and word in msg, (i, word, msg)
    good = TC.library_spec(TC.spec_dict())
    for field, value, word in (("max_apogee", math.nan, "max_apogee"), ("row_y", good.row_x, "listed twice")):
        s = TC.library_spec(TC.spec_dict())
        setattr(s, field, value)
        rc, msg = call_entry(lib, entry, s, state=None)
        assert rc == -1 and word in msg
    for first, word in (([0, 2, 5], "fewer than 3 vertices"), ([1, 4, 7], "zone_first"), ([0, 3, 2], "zone_first"), ([0, 4, 257], "more than 256")):
        s = TC.library_spec(TC.spec_dict())
        s.zone_first[0], s.zone_first[1], s.zone_first[2] = first
        rc, msg = call_entry(lib, entry, s, state=None)
        assert rc == -1 and word in msg, (first, msg)
    s = TC.library_spec(TC.spec_dict())
    s.zone_y[5] = math.inf
    rc, msg = call_entry(lib, entry, s, state=None)
    assert rc == -1 and "zone_y[5]" in msg
    # behind the spec: the pointers, the window, the context last
    if entry == "words":
        assert lib.erpl_mc_tally_words(C.byref(good), None) == -1 and "words is NULL" in lib.erpl_mc_last_error().decode()
        return
    first_pointer = "dst" if entry.startswith("merge") else "state"
    rc, msg = call_entry(lib, entry, good, state=None, other=None, summary=None, ld=-1, n=0, first_id=-1)
    assert rc == -1 and f"{first_pointer} is NULL" in msg
    if entry.startswith("add"):
        for kw, word in ((dict(summary=None, ld=-1, n=0, first_id=-1), "summary is NULL"), (dict(ld=-1, n=0, first_id=-1), "n = 0"),
                         (dict(ld=-1, n=-3, first_id=-1), "n = -3"), (dict(ld=-1, n=2 ** 31, first_id=-1), "2^31 - 1"),
                         (dict(ld=7, n=8, first_id=-1), "ld = 7"),
                         (dict(ld=8, n=8, first_id=-1), "first_id = -1"), (dict(ld=8, n=8, first_id=2 ** 63 - 8), "overflows")):
            rc, msg = call_entry(lib, entry, good, **kw)
            assert rc == -1 and word in msg, (kw, msg)
    elif entry.startswith("merge"):
        rc, msg = call_entry(lib, entry, good, other=None)
        assert rc == -1 and "src is NULL" in msg
    else:
        rc, msg = call_entry(lib, entry, good, result="NULL")
        assert rc == -1 and "result is NULL" in msg
    if entry in ("add", "merge", "result"):
        rc, msg = call_entry(lib, entry, good)
        assert rc == -1 and "ctx is NULL" in msg


def test_tally_check_builds_and_passes():
    """The header alone on the host: layout, canonical accumulators, splits and merges of a fixed table giving equal bytes."""
    subprocess.run(["make", "-C", CSRC, "erpl_tally_check"], check=True, capture_output=True)
    out = subprocess.run([os.path.join(CSRC, "erpl_tally_check")], capture_output=True, text=True)
    assert out.returncode == 0 and "erpl_tally_check ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ the rule, on the host
@pytest.mark.parametrize("n", TC.SIZES)
def test_host_tally_equals_the_restatement(n):
    d = TC.spec_dict()
    spec = TC.library_spec(d)
    summary, status = TC.table(n)
    check_against_ref(d, spec, host_tally(spec, [(summary, status, 1000)]), R.tally(d, summary, status, 1000))


@pytest.mark.parametrize("k,n", [(0, 257), (1, 257), (64, 63), (64, 1025)])
def test_extremes_for_every_k_also_with_fewer_than_k_counted_values(k, n):
    d = TC.spec_dict(k=k)
    spec = TC.library_spec(d)
    summary, status = TC.table(n, seed=11)
    check_against_ref(d, spec, host_tally(spec, [(summary, None, 2 ** 40)]), R.tally(d, summary, None, 2 ** 40))


def test_bins_of_one_and_of_1024_and_no_zones():
    d = TC.spec_dict(bins=(1, 1024, 1024, 1, 1024), zones=False)
    spec = TC.library_spec(d)
    summary, status = TC.table(1025, seed=3)
    check_against_ref(d, spec, host_tally(spec, [(summary, status, 0)]), R.tally(d, summary, status, 0))


def test_a_grid_of_256_by_200_cells():
    d = TC.spec_dict(grid=TC.BIG_GRID)
    spec = TC.library_spec(d)
    summary, status = TC.table(1025, seed=9)
    got = check_against_ref(d, spec, host_tally(spec, [(summary, status, 0)]), R.tally(d, summary, status, 0))
    assert np.count_nonzero(got["grid_counts"]) > 500


def test_a_window_where_every_sample_is_an_outlier():
    d = TC.spec_dict()
    spec = TC.library_spec(d)
    summary, status = TC.table(65, all_outliers=True)
    state = host_tally(spec, [(summary, status, 0)])
    got = check_against_ref(d, spec, state, R.tally(d, summary, status, 0))
    assert got["result"].n_valid == 0 and got["result"].grid_counted == 0 and not state[16:].any()


def test_exact_sums_of_an_ill_conditioned_row():
    """{1e300, 1.0, -1e300, 2^-60, ...} shuffled: sum_d is math.fsum's, sum_d2 the correctly rounded Fraction sum, and the
    |d| >= 2^500 entries are counted in moment_skipped and nowhere in the sums."""
    d = TC.spec_dict()
    spec = TC.library_spec(d)
    rs = np.random.RandomState(5)
    values = np.array(TC.EXACT * 20)
    rs.shuffle(values)
    summary, _ = TC.table(values.size, seed=13)
    summary[TC.APOGEE], summary[TC.RANGE], summary[TC.FLIGHT_TIME] = 1000.0, 100.0, 100.0    # every sample valid
    summary[TC.MAX_SPEED] = values
    res = analysis.tally_result_host(spec, host_tally(spec, [(summary, None, 0)]))["result"].row[3]
    kept = [float(v) for v in values if abs(v) < 2.0 ** 500]
    from fractions import Fraction
    want2 = float(sum((Fraction(v) ** 2 if abs(v) >= 2.0 ** -485 else Fraction(v * v) for v in kept), Fraction(0)))
    assert res.count == values.size and res.moment_skipped == values.size - len(kept) == 20 * 4
    assert res.sum_d == math.fsum(kept) and res.sum_d2 == want2
    assert res.sum_d != float(np.sum(kept)) or res.sum_d2 != float(np.sum(np.square(kept)))   # a running double sum is not it


def test_the_bytes_of_the_state_do_not_depend_on_splits_order_or_merge_tree():
    d = TC.spec_dict(k=64)
    spec = TC.library_spec(d)
    n = 1025
    summary, status = TC.table(n)
    cols = lambda a, b: (np.ascontiguousarray(summary[:, a:b]), status[a:b].copy(), 77 + a)
    one = host_tally(spec, [cols(0, n)])
    each = host_tally(spec, [cols(i, i + 1) for i in range(n)])
    back = host_tally(spec, [cols(i, i + 1) for i in reversed(range(n))])
    cut = [0, 1, 64, 129, 700, n]
    piece = [host_tally(spec, [cols(cut[p], cut[p + 1])]) for p in range(5)]
    analysis.tally_merge_host(spec, piece[3], piece[4])
    analysis.tally_merge_host(spec, piece[3], piece[1])
    analysis.tally_merge_host(spec, piece[0], piece[2])
    tree = np.zeros_like(one)
    analysis.tally_merge_host(spec, tree, piece[3])
    analysis.tally_merge_host(spec, tree, piece[0])
    assert one.tobytes() == each.tobytes() == back.tobytes() == tree.tobytes()
    assert one.any() and not np.array_equal(one, piece[0])
    check_against_ref(d, spec, tree, R.tally(d, summary, status, 77))


def test_result_refuses_a_count_past_2_62_and_reports_incomplete_samples(lib):
    d = TC.spec_dict()
    spec = TC.library_spec(d)
    summary, status = TC.table(64)
    state = host_tally(spec, [(summary, status, 0)])
    res = _abi.ErplTally()
    over = state.copy()
    over[0] = 2 ** 62 + 1
    assert lib.erpl_mc_tally_result_host(C.byref(spec), C.c_void_p(over.ctypes.data), C.byref(res), None, None) == -1
    assert "2^62" in lib.erpl_mc_last_error().decode()
    status[5] |= _abi.ST_INCOMPLETE
    state = host_tally(spec, [(summary, status, 0)])
    assert lib.erpl_mc_tally_result_host(C.byref(spec), C.c_void_p(state.ctypes.data), C.byref(res), None, None) == _abi.ERR_INCOMPLETE
    assert res.n == 64 and res.n_incomplete == 1     # with the result filled


def test_tally_statistics_shapes_the_result():
    d = TC.spec_dict()
    spec = TC.library_spec(d)
    summary, status = TC.table(1025)
    out = analysis.tally_statistics(analysis.tally_result_host(spec, host_tally(spec, [(summary, status, 0)])))
    ref = R.tally(d, summary, status, 0)
    assert out["n_samples"] == ref["n_valid"] and out["n_outliers"] == ref["n"] - ref["n_valid"]
    rng = out["rows"]["range"]
    assert set(("mean", "std", "min", "max", "percentiles")) <= set(out["range"])
    assert np.array_equal(rng["histogram"]["edges"], np.linspace(0.0, 2400.0, 51)) and rng["histogram"]["counts"].sum() == rng["count"]
    for t, want in zip(rng["exceedance"], ref["rows"][1]["exceed"]):
        assert t["count"] == want and t["probability"] == want / rng["count"]
        assert t["interval"] == analysis.wilson_interval(want, rng["count"], 0.95)
    for z, want in zip(out["zones"], ref["zone_inside"]):
        assert z["inside"] == want and z["interval"] == analysis.wilson_interval(want, ref["grid_counted"], 0.95)
    assert rng["largest"][0][0] == rng["max"] and len(rng["smallest"]) == d["k"]


def test_exceedance_figure_draws_the_tail():
    from erpl_monte_carlo_sim_amd import plots
    d = TC.spec_dict()
    spec = TC.library_spec(d)
    summary, status = TC.table(1025)
    out = analysis.tally_statistics(analysis.tally_result_host(spec, host_tally(spec, [(summary, status, 0)])))
    fig = plots.exceedance_figure(out, row="apogee_altitude")
    ax = fig.axes[0]
    assert ax.get_yscale() == "log" and ax.get_xlabel() == "apogee_altitude" and "exceedance" in ax.get_title()
    steps = ax.lines[0]
    y = np.asarray(steps.get_ydata())
    assert np.all(np.diff(y) <= 0) and y[0] <= 1.0 and y.min() > 0.0           # a complementary distribution, no zero on a log axis
    points = ax.lines[1]
    assert len(points.get_xdata()) == d["k"] and points.get_xdata()[0] == out["rows"]["apogee_altitude"]["max"]
    assert len(ax.collections) == 1                                              # the Wilson band
    assert sum(1 for line in ax.lines[2:]) == len(d["thresholds"][0])            # one marker per threshold
    fig.canvas.draw()
