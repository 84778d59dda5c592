"""Every refusal of the statistics entry points that needs no context, as (case id -> return code, whole
erpl_mc_last_error text): what tools/record_stats_refusals.py records into tests/golden/stats_refusals.json and what
test_stats_refusals.py compares.  One case per erpl_fail call site of csrc/erpl_stats_api.hip that comes before any device
work - the indexed and the unindexed spelling where a check has both - and the `ctx is NULL` that ends every entry point.
The context is NULL throughout and the pointers are a dummy that is never dereferenced."""
import ctypes as C

from erpl_monte_carlo_sim_amd import _abi

DUMMY = 0x1000
NAN, INF = float("nan"), float("inf")

# entry point: (spec, result, its arguments in order); every pointer not named in OPTIONAL is DUMMY, n is 8
ENTRIES = {
    "analyze": ("ErplAnalysisSpec", "ErplAnalysis", ("summary", "status", "n", "spec", "result", "reasons", "stream")),
    "histogram": ("ErplHistSpec", "ErplHistResult", ("summary", "mask", "n", "spec", "edges", "counts", "result", "stream")),
    "histogram_xy": ("ErplHist2dSpec", "ErplHist2dResult",
                     ("summary", "mask", "n", "spec", "edges_x", "edges_y", "counts", "result", "stream")),
    "dispersion": ("ErplDispersionSpec", "ErplDispersion", ("summary", "mask", "n", "spec", "result", "miss", "stream")),
    "correlation": ("ErplCorrSpec", "ErplCorrResult",
                    ("factors", "summary", "mask", "n", "spec", "result", "corr", "rank_corr", "ranks_out", "stream")),
    "bootstrap": ("ErplBootSpec", "ErplBootstrap",
                  ("summary", "extra", "mask", "n", "spec", "result", "replicates_out", "stream")),
    "impact_density": ("ErplDensitySpec", "ErplDensity",
                       ("summary", "mask", "n", "spec", "grid_x", "grid_y", "density", "result", "sample_density", "stream")),
}
DEFAULTS = {"analyze": "analysis", "histogram_xy": None}   # erpl_mc_<name>_defaults where it is not the entry's own name
OPTIONAL = ("status", "mask", "reasons", "miss", "rank_corr", "ranks_out", "extra", "replicates_out", "sample_density", "stream",
            "corr")

TRI = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]


def zones(*polys, **first):
    """Spec edits for the polygons; first = {index: value} overrides zone_first afterwards."""
    edits, at = {"n_zones": len(polys)}, 0
    for z, poly in enumerate(polys):
        edits[f"zone_first[{z}]"] = at
        for x, y in poly:
            if at < _abi.DENSITY_MAX_VERTICES:
                edits[f"zone_x[{at}]"], edits[f"zone_y[{at}]"] = x, y
            at += 1
    edits[f"zone_first[{len(polys)}]"] = at
    edits.update({f"zone_first[{k[1:]}]": v for k, v in first.items()})
    return edits


# (case id, entry point, spec edits or None for a NULL spec, argument overrides)
CASES = [
    # ---- erpl_mc_analyze
    ("analyze/spec_null", "analyze", None, {}),
    *[(f"analyze/{f}_nan", "analyze", {f: NAN}, {}) for f in ("max_apogee", "min_apogee", "max_range", "max_flight_time",
                                                               "energy_apogee")],
    ("analyze/n_rows_high", "analyze", {"n_rows": 17}, {}),
    ("analyze/n_rows_low", "analyze", {"n_rows": -1}, {}),
    ("analyze/row_high", "analyze", {"rows[1]": 16}, {}),
    ("analyze/row_low", "analyze", {"rows[0]": -1}, {}),
    ("analyze/row_twice", "analyze", {"rows[2]": _abi.SUM_APOGEE_ALT}, {}),
    ("analyze/n_q_high", "analyze", {"n_q": 9}, {}),
    ("analyze/n_q_low", "analyze", {"n_q": -1}, {}),
    ("analyze/q_high", "analyze", {"q[3]": 1.01}, {}),
    ("analyze/q_nan", "analyze", {"q[0]": NAN}, {}),
    ("analyze/n_zero", "analyze", {}, {"n": 0}),
    ("analyze/n_negative", "analyze", {}, {"n": -5}),
    ("analyze/summary_null", "analyze", {}, {"summary": None}),
    ("analyze/result_null", "analyze", {}, {"result": None}),
    ("analyze/ctx_null", "analyze", {}, {}),
    ("analyze/order", "analyze", {"max_range": NAN, "n_rows": 17, "n_q": 9}, {"n": 0, "summary": None, "result": None}),
    # ---- erpl_mc_histogram
    ("histogram/spec_null", "histogram", None, {}),
    ("histogram/n_rows_zero", "histogram", {"n_rows": 0}, {}),
    ("histogram/n_rows_high", "histogram", {"n_rows": 17}, {}),
    ("histogram/row_high", "histogram", {"rows[2]": 16}, {}),
    ("histogram/row_twice", "histogram", {"rows[1]": _abi.SUM_APOGEE_ALT}, {}),
    ("histogram/bins_zero", "histogram", {"bins[1]": 0}, {}),
    ("histogram/bins_high", "histogram", {"bins[2]": 1025}, {}),
    ("histogram/range_half_nan", "histogram", {"lo[1]": 0.0}, {}),
    ("histogram/range_half_nan_hi", "histogram", {"hi[0]": 2.5}, {}),
    ("histogram/range_infinite", "histogram", {"lo[2]": -INF, "hi[2]": 1.0}, {}),
    ("histogram/range_overflows", "histogram", {"lo[0]": -1.5e308, "hi[0]": 1.5e308}, {}),
    ("histogram/range_reversed", "histogram", {"lo[1]": 2.0, "hi[1]": 1.0}, {}),
    ("histogram/n_zero", "histogram", {}, {"n": 0}),
    *[(f"histogram/{p}_null", "histogram", {}, {p: None}) for p in ("summary", "edges", "counts", "result")],
    ("histogram/ctx_null", "histogram", {}, {}),
    ("histogram/order", "histogram", {"bins[0]": 0, "lo[0]": 1.0}, {"n": 0, "summary": None, "edges": None}),
    # ---- erpl_mc_histogram_xy (no defaults call: the fields are set here)
    ("histogram_xy/spec_null", "histogram_xy", None, {}),
    ("histogram_xy/row_x_high", "histogram_xy", {"row_x": 16}, {}),
    ("histogram_xy/row_y_low", "histogram_xy", {"row_y": -1}, {}),
    ("histogram_xy/row_twice", "histogram_xy", {"row_y": _abi.SUM_IMPACT_X}, {}),
    ("histogram_xy/bins_x_zero", "histogram_xy", {"bins_x": 0}, {}),
    ("histogram_xy/bins_x_high", "histogram_xy", {"bins_x": 257}, {}),
    ("histogram_xy/bins_y_zero", "histogram_xy", {"bins_y": 0}, {}),
    ("histogram_xy/bins_y_high", "histogram_xy", {"bins_y": 257}, {}),
    ("histogram_xy/range_x_half_nan", "histogram_xy", {"lo_x": 0.0}, {}),
    ("histogram_xy/range_y_half_nan", "histogram_xy", {"hi_y": 1.0}, {}),
    ("histogram_xy/range_x_infinite", "histogram_xy", {"lo_x": 0.0, "hi_x": INF}, {}),
    ("histogram_xy/range_y_reversed", "histogram_xy", {"lo_y": 2.0, "hi_y": -2.0}, {}),
    ("histogram_xy/n_zero", "histogram_xy", {}, {"n": 0}),
    *[(f"histogram_xy/{p}_null", "histogram_xy", {}, {p: None}) for p in ("summary", "edges_x", "edges_y", "counts", "result")],
    ("histogram_xy/ctx_null", "histogram_xy", {}, {}),
    # ---- erpl_mc_dispersion
    ("dispersion/spec_null", "dispersion", None, {}),
    ("dispersion/row_x_high", "dispersion", {"row_x": 16}, {}),
    ("dispersion/row_y_low", "dispersion", {"row_y": -2}, {}),
    ("dispersion/row_twice", "dispersion", {"row_y": _abi.SUM_IMPACT_X}, {}),
    ("dispersion/centre", "dispersion", {"centre": 2}, {}),
    ("dispersion/centre_nan", "dispersion", {"cx": NAN}, {}),
    ("dispersion/centre_inf", "dispersion", {"cy": -INF}, {}),
    ("dispersion/n_levels_high", "dispersion", {"n_levels": 9}, {}),
    ("dispersion/n_levels_low", "dispersion", {"n_levels": -1}, {}),
    ("dispersion/level_one", "dispersion", {"level[1]": 1.0}, {}),
    ("dispersion/level_nan", "dispersion", {"level[0]": NAN}, {}),
    ("dispersion/n_q_high", "dispersion", {"n_q": 9}, {}),
    ("dispersion/q_low", "dispersion", {"q[2]": -0.01}, {}),
    ("dispersion/n_zero", "dispersion", {}, {"n": 0}),
    ("dispersion/summary_null", "dispersion", {}, {"summary": None}),
    ("dispersion/result_null", "dispersion", {}, {"result": None}),
    ("dispersion/ctx_null", "dispersion", {}, {}),
    # ---- erpl_mc_correlation
    ("correlation/spec_null", "correlation", None, {}),
    ("correlation/n_factors_zero", "correlation", {"n_factors": 0}, {}),
    ("correlation/n_factors_high", "correlation", {"n_factors": 33}, {}),
    ("correlation/n_rows_zero", "correlation", {"n_rows": 0}, {}),
    ("correlation/n_rows_high", "correlation", {"n_rows": 17}, {}),
    ("correlation/row_high", "correlation", {"rows[0]": 16}, {}),
    ("correlation/row_twice", "correlation", {"rows[2]": _abi.SUM_RANGE}, {}),
    ("correlation/ranks", "correlation", {"ranks": 2}, {}),
    ("correlation/rank_corr_without_ranks", "correlation", {"ranks": 0}, {"rank_corr": DUMMY}),
    ("correlation/ranks_out_without_ranks", "correlation", {"ranks": 0}, {"ranks_out": DUMMY}),
    ("correlation/n_zero", "correlation", {}, {"n": 0}),
    ("correlation/n_beyond_32_bits", "correlation", {}, {"n": 2 ** 32}),
    *[(f"correlation/{p}_null", "correlation", {}, {p: None}) for p in ("factors", "summary", "result")],
    ("correlation/ctx_null", "correlation", {}, {}),
    ("correlation/ctx_null_no_ranks_wide", "correlation", {"ranks": 0}, {"n": 2 ** 32}),
    # ---- erpl_mc_bootstrap: pointers, n, then the spec
    ("bootstrap/spec_null", "bootstrap", None, {"n": 0, "summary": None, "result": None}),
    ("bootstrap/summary_null", "bootstrap", {"n_rows": 0}, {"n": 0, "summary": None, "result": None}),
    ("bootstrap/result_null", "bootstrap", {"n_rows": 0}, {"n": 0, "result": None}),
    ("bootstrap/n_zero", "bootstrap", {"n_rows": 0}, {"n": 0}),
    ("bootstrap/n_negative", "bootstrap", {"n_rows": 0}, {"n": -5}),
    ("bootstrap/n_beyond_31_bits", "bootstrap", {"n_rows": 0}, {"n": 2 ** 31}),
    ("bootstrap/n_rows_zero", "bootstrap", {"n_rows": 0, "n_q": 9}, {}),
    ("bootstrap/n_rows_high", "bootstrap", {"n_rows": 5, "n_q": 9}, {}),
    ("bootstrap/n_q_high", "bootstrap", {"n_q": 9, "replicates": 0}, {}),
    ("bootstrap/n_q_low", "bootstrap", {"n_q": -1, "replicates": 0}, {}),
    ("bootstrap/replicates_zero", "bootstrap", {"replicates": 0, "rows[0]": 17}, {}),
    ("bootstrap/replicates_high", "bootstrap", {"replicates": 65537, "rows[0]": 17}, {}),
    ("bootstrap/row_high", "bootstrap", {"rows[1]": 17, "q[0]": 2.0}, {}),
    ("bootstrap/row_low", "bootstrap", {"rows[1]": -1, "q[0]": 2.0}, {}),
    ("bootstrap/row_twice", "bootstrap", {"rows[2]": _abi.SUM_APOGEE_ALT, "q[0]": 2.0}, {}),
    ("bootstrap/extra_null", "bootstrap", {"rows[1]": _abi.BOOT_ROW_EXTRA, "q[0]": 2.0}, {}),
    ("bootstrap/row_twice_before_extra", "bootstrap", {"rows[0]": 16, "rows[2]": 16}, {}),
    ("bootstrap/q_high", "bootstrap", {"q[3]": 1.01, "level": 1.0}, {}),
    ("bootstrap/q_nan", "bootstrap", {"q[4]": NAN, "level": 1.0}, {}),
    ("bootstrap/level_one", "bootstrap", {"level": 1.0}, {}),
    ("bootstrap/level_nan", "bootstrap", {"level": NAN}, {}),
    ("bootstrap/ctx_null", "bootstrap", {}, {}),
    ("bootstrap/ctx_null_at_the_limits", "bootstrap", {"n_rows": 4, "rows[0]": 15, "rows[1]": 0, "rows[2]": 16, "rows[3]": 7,
                                                        "n_q": 8, "q[5]": 0.1, "q[6]": 0.9, "q[7]": 1.0, "replicates": 65536},
     {"n": 2 ** 31 - 1, "extra": DUMMY, "replicates_out": DUMMY}),
    # ---- erpl_mc_impact_density
    ("impact_density/spec_null", "impact_density", None, {}),
    ("impact_density/row_x_high", "impact_density", {"row_x": 16}, {}),
    ("impact_density/row_y_low", "impact_density", {"row_y": -1}, {}),
    ("impact_density/row_twice", "impact_density", {"row_y": _abi.SUM_IMPACT_X}, {}),
    ("impact_density/nodes_x_low", "impact_density", {"nodes_x": 1}, {}),
    ("impact_density/nodes_x_high", "impact_density", {"nodes_x": 513}, {}),
    ("impact_density/nodes_y_low", "impact_density", {"nodes_y": -4}, {}),
    ("impact_density/nodes_y_high", "impact_density", {"nodes_y": 513}, {}),
    ("impact_density/range_x_half_nan", "impact_density", {"lo_x": 0.0}, {}),
    ("impact_density/range_y_half_nan", "impact_density", {"hi_y": 1.0}, {}),
    ("impact_density/range_x_infinite", "impact_density", {"lo_x": -INF, "hi_x": 1.0}, {}),
    ("impact_density/range_x_reversed", "impact_density", {"lo_x": 2.0, "hi_x": 1.0}, {}),
    ("impact_density/range_y_empty", "impact_density", {"lo_y": 5.0, "hi_y": 5.0}, {}),
    ("impact_density/pad_negative", "impact_density", {"pad": -0.5}, {}),
    ("impact_density/pad_nan", "impact_density", {"pad": NAN}, {}),
    ("impact_density/bandwidth", "impact_density", {"bandwidth": 2}, {}),
    ("impact_density/bw_scale_zero", "impact_density", {"bw_scale": 0.0}, {}),
    ("impact_density/bw_scale_inf", "impact_density", {"bw_scale": INF}, {}),
    ("impact_density/matrix_singular", "impact_density", {"bandwidth": _abi.BW_MATRIX, "h_xx": 1.0, "h_xy": 1.0, "h_yy": 1.0}, {}),
    ("impact_density/matrix_nan", "impact_density", {"bandwidth": _abi.BW_MATRIX, "h_xx": NAN, "h_xy": 0.0, "h_yy": 1.0}, {}),
    ("impact_density/n_levels_high", "impact_density", {"n_levels": 9}, {}),
    ("impact_density/n_levels_low", "impact_density", {"n_levels": -1}, {}),
    ("impact_density/level_zero", "impact_density", {"level[2]": 0.0}, {}),
    ("impact_density/level_nan", "impact_density", {"level[0]": NAN}, {}),
    ("impact_density/n_zones_high", "impact_density", {"n_zones": 9}, {}),
    ("impact_density/n_zones_low", "impact_density", {"n_zones": -1}, {}),
    ("impact_density/zone_first_0", "impact_density", zones(TRI, _0=1), {}),
    ("impact_density/zone_first_decreasing", "impact_density", zones(TRI, TRI, _2=2), {}),
    ("impact_density/zone_two_vertices", "impact_density", zones(TRI, [(0.0, 0.0), (1.0, 1.0)]), {}),
    ("impact_density/zone_257_vertices", "impact_density", zones([(float(k), float(k * k)) for k in range(257)]), {}),
    ("impact_density/zone_vertex_nan", "impact_density", zones(TRI, [(0.0, 0.0), (NAN, 0.0), (0.0, 1.0)]), {}),
    ("impact_density/zone_vertex_inf", "impact_density", zones([(0.0, 0.0), (1.0, 0.0), (0.0, INF)]), {}),
    ("impact_density/n_zero", "impact_density", {}, {"n": 0}),
    ("impact_density/n_beyond_31_bits", "impact_density", {}, {"n": 2 ** 31}),
    *[(f"impact_density/{p}_null", "impact_density", {}, {p: None}) for p in ("summary", "grid_x", "grid_y", "density", "result")],
    ("impact_density/ctx_null", "impact_density", {}, {}),
    ("impact_density/order", "impact_density", {"n_zones": 9, "level[0]": 2.0, "pad": -1.0}, {"n": 0, "summary": None}),
]

# erpl_mc_bootstrap_indices(seed, replicate, m, first, count, out): overrides of (0, 0, 8, 0, 8, a buffer of 8)
INDEX_CASES = [
    ("bootstrap_indices/out_null", {"out": None}),
    ("bootstrap_indices/m_zero", {"m": 0, "count": 0}),
    ("bootstrap_indices/m_beyond_31_bits", {"m": 2 ** 31, "count": 0}),
    ("bootstrap_indices/replicate_negative", {"replicate": -1}),
    ("bootstrap_indices/replicate_beyond_32_bits", {"replicate": 2 ** 32}),
    ("bootstrap_indices/first_negative", {"first": -1, "count": 1}),
    ("bootstrap_indices/count_negative", {"count": -1}),
    ("bootstrap_indices/window_beyond_m", {"first": 1, "count": 8}),
    ("bootstrap_indices/first_beyond_m", {"first": 9, "count": 0}),
]


def _set(spec, key, value):
    if key.endswith("]"):
        name, idx = key[:-1].split("[")
        getattr(spec, name)[int(idx)] = value
    else:
        setattr(spec, key, value)


def make_spec(lib, entry):
    spec = getattr(_abi, ENTRIES[entry][0])()
    name = DEFAULTS.get(entry, entry)
    if name is None:       # erpl_mc_histogram_xy has no defaults call
        spec.row_x, spec.row_y, spec.bins_x, spec.bins_y = _abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y, 50, 40
        spec.lo_x = spec.hi_x = spec.lo_y = spec.hi_y = NAN
    else:
        assert getattr(lib, f"erpl_mc_{name}_defaults")(C.byref(spec)) == 0
    if entry == "correlation":
        spec.n_factors = 2
    return spec


def run_case(lib, entry, edits, over):
    spec_name, result_name, names = ENTRIES[entry]
    assert set(over) <= set(names), (entry, over)
    spec = None
    if edits is not None:
        spec = make_spec(lib, entry)
        for k, v in edits.items():
            _set(spec, k, v)
    result = getattr(_abi, result_name)()
    args = []
    for name in names:
        if name == "spec":
            args.append(C.byref(spec) if spec is not None else None)
        elif name == "result":
            args.append(None if "result" in over else C.byref(result))
        elif name == "n":
            args.append(over.get("n", 8))
        else:
            v = over.get(name, None if name in OPTIONAL else DUMMY)
            args.append(None if v is None else C.c_void_p(v))
    rc = getattr(lib, f"erpl_mc_{entry}")(None, *args)
    return [int(rc), lib.erpl_mc_last_error().decode()]


def collect(lib):
    """{case id: [rc, message]} of every case, defaults calls with a NULL spec included."""
    rec = {}
    for name in ("analysis", "histogram", "dispersion", "correlation", "bootstrap", "impact_density"):
        rc = getattr(lib, f"erpl_mc_{name}_defaults")(None)
        rec[f"{name}_defaults/spec_null"] = [int(rc), lib.erpl_mc_last_error().decode()]
    for cid, entry, edits, over in CASES:
        assert cid not in rec, cid
        rec[cid] = run_case(lib, entry, edits, over)
    buf = (C.c_int64 * 8)()
    lib.erpl_mc_bootstrap_indices.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    for cid, over in INDEX_CASES:
        a = dict(seed=0, replicate=0, m=8, first=0, count=8, out=buf)
        a.update(over)
        rc = lib.erpl_mc_bootstrap_indices(a["seed"], a["replicate"], a["m"], a["first"], a["count"], a["out"])
        rec[cid] = [int(rc), lib.erpl_mc_last_error().decode()]
    return rec

