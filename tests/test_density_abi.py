"""erpl_mc_impact_density and erpl_mc_impact_density_defaults at the C boundary, as far as it goes without a GPU: struct
layouts against gcc, the defaults, every argument check (they come before any device work and look at the context last, so
a NULL context and a dummy pointer that is never dereferenced show them all), the host-side refusal of the engine method,
the Wilson interval against its closed form and the figure drawn from a hand-made result dict."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis, plots

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
DUMMY = H.DUMMY

STRUCTS = (("erpl_density_spec", "ErplDensitySpec"), ("erpl_density", "ErplDensity"))
MACROS = (("ERPL_DENSITY_MAX_NODES", _abi.DENSITY_MAX_NODES), ("ERPL_DENSITY_MAX_LEVELS", _abi.DENSITY_MAX_LEVELS),
          ("ERPL_DENSITY_MAX_ZONES", _abi.DENSITY_MAX_ZONES),
          ("ERPL_DENSITY_MAX_VERTICES", _abi.DENSITY_MAX_VERTICES), ("ERPL_BW_SCOTT", _abi.BW_SCOTT),
          ("ERPL_BW_MATRIX", _abi.BW_MATRIX))


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and the offset of EVERY field of the two new ctypes mirrors == what gcc sees in include/erpl_mc.h."""
    H.check_struct_layouts(tmp_path, STRUCTS, MACROS)
    assert (_abi.DENSITY_MAX_NODES, _abi.DENSITY_MAX_ZONES, _abi.DENSITY_MAX_VERTICES) == (512, 8, 256)
    assert _abi.ABI_VERSION == 4


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_impact_density_defaults", "erpl_mc_impact_density"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def defaults(lib):
    spec = _abi.ErplDensitySpec()
    assert lib.erpl_mc_impact_density_defaults(C.byref(spec)) == 0
    return spec


def with_zones(lib, polys):
    spec, at = defaults(lib), 0
    spec.n_zones = len(polys)
    for z, poly in enumerate(polys):
        spec.zone_first[z] = at
        for x, y in poly:
            if at < _abi.DENSITY_MAX_VERTICES:   # (the arrays hold no more; zone_first alone says there are)
                spec.zone_x[at], spec.zone_y[at] = x, y
            at += 1
    spec.zone_first[len(polys)] = at
    return spec


def test_defaults(lib):
    s = defaults(lib)
    assert (s.row_x, s.row_y) == (_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y)
    assert (s.nodes_x, s.nodes_y) == (128, 128)
    assert all(math.isnan(v) for v in (s.lo_x, s.hi_x, s.lo_y, s.hi_y)) and s.pad == 3.0
    assert s.bandwidth == _abi.BW_SCOTT and s.bw_scale == 1.0
    assert s.n_levels == 3 and list(s.level[:3]) == [0.5, 0.9, 0.99]
    assert s.n_zones == 0
    assert lib.erpl_mc_impact_density_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_argument_checks_come_before_any_device_work(lib):
    res = _abi.ErplDensity()

    def call(spec, n=8, summary=DUMMY, grid_x=DUMMY, grid_y=DUMMY, density=DUMMY, result=res):
        rc = lib.erpl_mc_impact_density(None, summary, None, n, C.byref(spec) if spec is not None else None, grid_x, grid_y,
                                        density, C.byref(result) if result is not None else None, None, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(words, **fields):
        spec = defaults(lib)
        for k, v in fields.items():
            setattr(spec, k, v)
        rc, msg = call(spec)
        assert rc == -1 and all(w in msg for w in words), (fields, msg)

    rc, msg = call(None)
    assert rc == -1 and "spec" in msg
    for n in (0, -3, 1 << 31):
        rc, msg = call(defaults(lib), n=n)
        assert rc == -1 and f"n = {n}" in msg
    # rows, and rows given twice
    refused(("row_x", "16"), row_x=16)
    refused(("row_y", "-1"), row_y=-1)
    refused(("twice",), row_y=_abi.SUM_IMPACT_X)
    # nodes 1 and 513
    for field in ("nodes_x", "nodes_y"):
        for bad in (1, 513, 0, -4):
            refused((field, str(bad)), **{field: bad})
    # a half-NaN range, and lo >= hi
    refused(("lo_x", "hi_x"), lo_x=0.0)
    refused(("lo_y", "hi_y"), hi_y=1.0)
    refused(("lo_x", "hi_x"), lo_x=2.0, hi_x=1.0)
    refused(("lo_y", "hi_y"), lo_y=5.0, hi_y=5.0)
    refused(("lo_x", "hi_x"), lo_x=-math.inf, hi_x=1.0)
    # pad negative or NaN
    for bad in (-0.5, NAN, math.inf):
        refused(("pad",), pad=bad)
    # the bandwidth
    refused(("bandwidth", "2"), bandwidth=2)
    for bad in (0.0, -1.0, NAN, math.inf):
        refused(("bw_scale",), bw_scale=bad)
    for hxx, hxy, hyy in ((1.0, 1.0, 1.0), (1.0, 2.0, 1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (NAN, 0.0, 1.0), (1.0, math.inf, 1.0)):
        refused(("h_xx", "h_xy", "h_yy"), bandwidth=_abi.BW_MATRIX, h_xx=hxx, h_xy=hxy, h_yy=hyy)
    # levels 0, 1 and NaN
    refused(("n_levels", "9"), n_levels=9)
    refused(("n_levels", "-1"), n_levels=-1)
    for bad in (0.0, 1.0, NAN, -0.2, 1.5):
        spec = defaults(lib)
        spec.level[2] = bad
        rc, msg = call(spec)
        assert rc == -1 and "level[2]" in msg, bad
    # zones
    refused(("n_zones", "9"), n_zones=9)
    refused(("n_zones", "-1"), n_zones=-1)
    tri = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]
    rc, msg = call(with_zones(lib, [tri, [(0.0, 0.0), (1.0, 1.0)]]))            # a zone with 2 vertices
    assert rc == -1 and "zone_first" in msg and "2 vertices" in msg
    rc, msg = call(with_zones(lib, [[(float(k), float(k * k)) for k in range(257)]]))   # 257 vertices
    assert rc == -1 and "zone_first[1]" in msg and "257" in msg and "256" in msg
    for bad in (NAN, math.inf):                                                 # a non-finite vertex
        rc, msg = call(with_zones(lib, [tri, [(0.0, 0.0), (bad, 0.0), (0.0, 1.0)]]))
        assert rc == -1 and "zone_x[4]" in msg
        rc, msg = call(with_zones(lib, [[(0.0, 0.0), (1.0, 0.0), (0.0, bad)]]))
        assert rc == -1 and "zone_y[2]" in msg
    spec = with_zones(lib, [tri, tri])                                          # decreasing zone_first
    spec.zone_first[2] = 2
    rc, msg = call(spec)
    assert rc == -1 and "zone_first[2]" in msg and "below" in msg
    spec = with_zones(lib, [tri])
    spec.zone_first[0] = 1
    rc, msg = call(spec)
    assert rc == -1 and "zone_first[0]" in msg
    # the pointers
    for name in ("summary", "grid_x", "grid_y", "density"):
        rc, msg = call(defaults(lib), **{name: None})
        assert rc == -1 and name in msg
    rc, msg = call(defaults(lib), result=None)
    assert rc == -1 and "result" in msg
    # everything in order - explicit ranges, a matrix, pad 0, 8 levels, 8 zones of 256 vertices together: only the context is left
    spec = with_zones(lib, [[(math.cos(0.2 * k + z), math.sin(0.2 * k + z)) for k in range(32)] for z in range(8)])
    spec.nodes_x, spec.nodes_y = 2, 512
    spec.lo_x, spec.hi_x, spec.lo_y, spec.hi_y = -1.0, 1.0, 0.0, 1e-300
    spec.pad = 0.0
    spec.bandwidth, spec.h_xx, spec.h_xy, spec.h_yy = _abi.BW_MATRIX, 2.0, -1.0, 1.0
    spec.bw_scale = NAN                                                        # not looked at with a matrix
    spec.n_levels = 8
    spec.level[:8] = [0.1 * (k + 1) for k in range(8)]
    rc, msg = call(spec)
    assert rc == -1 and "ctx" in msg
    rc, msg = call(defaults(lib))
    assert rc == -1 and "ctx" in msg


def test_engine_method_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.impact_density: the refusal is on the host, before the library is called (the
    engine here has no library and no context)."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.impact_density(eng, torch.zeros((16, 4), dtype=torch.float64))


def test_wilson_interval_against_its_closed_form():
    z = 1.959963984540054   # the standard normal quantile of 0.975
    lo, hi = analysis.wilson_interval(0, 50)
    assert lo == 0.0 and abs(hi - z * z / (50 + z * z)) < 1e-14            # k = 0: (0, z^2 / (n + z^2))
    lo, hi = analysis.wilson_interval(50, 50)
    assert hi == 1.0 and abs(lo - 50 / (50 + z * z)) < 1e-14                 # k = n: (n / (n + z^2), 1)
    k, n = 37, 120
    p = k / n
    centre = (p + z * z / (2 * n)) / (1 + z * z / n)
    half = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / (1 + z * z / n)
    lo, hi = analysis.wilson_interval(k, n)
    assert abs(lo - (centre - half)) < 1e-14 and abs(hi - (centre + half)) < 1e-14 and lo < p < hi
    z90 = 1.6448536269514722
    lo, hi = analysis.wilson_interval(0, 10, level=0.9)
    assert abs(hi - z90 * z90 / (10 + z90 * z90)) < 1e-14
    assert analysis.wilson_interval(0, 0) == (0.0, 1.0)
    with pytest.raises(ValueError):
        analysis.wilson_interval(5, 4)


def hand_made_result():
    gx, gy = np.linspace(-4.0, 6.0, 41), np.linspace(-3.0, 3.0, 25)
    dens = np.exp(-0.5 * ((gx[:, None] - 1.0) ** 2 / 2.0 + gy[None, :] ** 2)) / (2 * math.pi * math.sqrt(2.0))
    peak = float(dens.max())
    zones = [{"vertices": np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [0.0, 2.0]]), "inside": 31, "probability": 0.31,
              "interval": (0.228, 0.406)},
             {"vertices": np.array([[-3.0, -2.0], [-1.0, -2.0], [-2.0, 1.0]]), "inside": 0, "probability": 0.0,
              "interval": (0.0, 0.037)}]
    return {"count": 100, "solid": True, "grid_x": gx, "grid_y": gy, "density": dens, "peak": peak,
            "levels": [0.5, 0.9, 0.99], "thresholds": [0.5 * peak, 0.1 * peak, 0.01 * peak],
            "ranges": ((-4.0, 6.0), (-3.0, 3.0)), "zones": zones}


def test_figure_from_a_hand_made_result(tmp_path):
    from matplotlib.contour import ContourSet
    from matplotlib.patches import Polygon
    res = hand_made_result()
    fig = plots.impact_probability_figure(res)
    ax = fig.axes[0]
    sets = [c for c in ax.collections if isinstance(c, ContourSet)]
    filled = [c for c in sets if c.filled]
    lines = [c for c in sets if not c.filled]
    assert len(filled) == 1 and len(lines) == 1
    want = sorted(res["thresholds"])
    assert list(lines[0].levels) == want                       # the contour levels are the dict's thresholds
    assert list(filled[0].levels[:-1]) == want and filled[0].levels[-1] > res["peak"]
    outlines = [p for p in ax.patches if isinstance(p, Polygon)]
    assert len(outlines) == len(res["zones"])                  # one outline per zone
    for patch, z in zip(outlines, res["zones"]):
        assert np.array_equal(patch.get_xy()[:len(z["vertices"])], z["vertices"])
    labels = [t.get_text() for t in ax.get_legend().get_texts()]
    assert any("50 %" in s for s in labels) and any("90 %" in s for s in labels) and any("99 %" in s for s in labels)
    assert any("P = 0.31" in s for s in labels) and any("Launch site" in s for s in labels)
    path = plots.save_figure(fig, str(tmp_path), "monte_carlo_impact_probability.png")
    assert os.path.getsize(path) > 0
    # not solid: the zones and the launch site, no contours
    res["solid"], res["thresholds"] = False, [NAN] * 3
    res["density"] = np.full_like(res["density"], NAN)
    ax = plots.impact_probability_figure(res).axes[0]
    assert not [c for c in ax.collections if isinstance(c, ContourSet)]
    assert len([p for p in ax.patches if isinstance(p, Polygon)]) == 2
