"""erpl_mc_impact_density_weighted at the C boundary, as far as it goes without a GPU: the struct layout against gcc, every
argument check in the order of the header (they come before any device work and look at the context last, so a NULL context
and dummy pointers that are never dereferenced show them all), the workspace layout through erpl_stat_layout_table and the
host-side refusals of the engine method."""
import ctypes as C
import math
import os
import subprocess

import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
DUMMY = H.DUMMY
TABLE = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc", "erpl_stat_layout_table")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_struct_layout_matches_the_c_compiler(tmp_path):
    H.check_struct_layouts(tmp_path, (("erpl_density_w", "ErplDensityW"), ("erpl_density_spec", "ErplDensitySpec")),
                           (("ERPL_DENSITY_MAX_ZONES", _abi.DENSITY_MAX_ZONES), ("ERPL_DENSITY_MAX_LEVELS", _abi.DENSITY_MAX_LEVELS)))
    assert _abi.ABI_VERSION == 4


def test_the_symbol_is_declared_exported_and_documented(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    name = "erpl_mc_impact_density_weighted"
    assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc
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
            if at < _abi.DENSITY_MAX_VERTICES:
                spec.zone_x[at], spec.zone_y[at] = x, y
            at += 1
    spec.zone_first[len(polys)] = at
    return spec


def test_argument_checks_in_the_order_of_the_header(lib):
    res = _abi.ErplDensityW()
    names = ("summary", "grid_x", "grid_y", "density", "weights", "result")

    def call(spec, n=8, **ptr):
        p = {k: ptr.get(k, DUMMY) for k in names[:-1]}
        result = ptr.get("result", res)
        rc = lib.erpl_mc_impact_density_weighted(None, p["summary"], None, p["weights"], n, C.byref(spec) if spec is not None else None,
                                                 p["grid_x"], p["grid_y"], p["density"], C.byref(result) if result is not None else None,
                                                 None, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(words, n=8, **fields):
        spec = defaults(lib)
        for k, v in fields.items():
            setattr(spec, k, v)
        rc, msg = call(spec, n=n)
        assert rc == -1 and all(w in msg for w in words), (fields, msg)

    rc, msg = call(None)
    assert rc == -1 and "spec" in msg
    # the spec, field by field (the checks of erpl_mc_impact_density)
    refused(("row_x", "16"), row_x=16)
    refused(("row_y", "-1"), row_y=-1)
    refused(("twice",), row_y=_abi.SUM_IMPACT_X)
    for field in ("nodes_x", "nodes_y"):
        for bad in (1, 513):
            refused((field, str(bad)), **{field: bad})
    refused(("lo_x", "hi_x"), lo_x=0.0)
    refused(("lo_y", "hi_y"), lo_y=5.0, hi_y=5.0)
    for bad in (-0.5, NAN, math.inf):
        refused(("pad",), pad=bad)
    refused(("bandwidth", "2"), bandwidth=2)
    for bad in (0.0, NAN):
        refused(("bw_scale",), bw_scale=bad)
    refused(("h_xx", "h_xy", "h_yy"), bandwidth=_abi.BW_MATRIX, h_xx=1.0, h_xy=2.0, h_yy=1.0)
    refused(("n_levels", "9"), n_levels=9)
    spec = defaults(lib)
    spec.level[1] = 1.0
    rc, msg = call(spec)
    assert rc == -1 and "level[1]" in msg
    refused(("n_zones", "9"), n_zones=9)
    rc, msg = call(with_zones(lib, [[(0.0, 0.0), (1.0, 1.0)]]))
    assert rc == -1 and "2 vertices" in msg
    rc, msg = call(with_zones(lib, [[(0.0, 0.0), (NAN, 0.0), (0.0, 1.0)]]))
    assert rc == -1 and "zone_x[1]" in msg
    # a bad spec field is seen before a bad n, a bad n before a NULL pointer
    refused(("row_x",), n=0, row_x=16)
    for n in (0, -3, 1 << 31):
        rc, msg = call(defaults(lib), n=n, summary=None)
        assert rc == -1 and f"n = {n}" in msg
    # the pointers, in order: each one is reported although every later one is NULL too
    for k, name in enumerate(names):
        rc, msg = call(defaults(lib), **{later: None for later in names[k:]})
        assert rc == -1 and f"{name} is NULL" in msg, (name, msg)
    # everything in order: only the context is left
    rc, msg = call(defaults(lib))
    assert rc == -1 and "ctx" in msg


def test_the_workspace_has_its_own_row_and_leaves_the_map_s_alone():
    ask = "wdens 1000 4096 1 0 300\nwdens 1000 4096 1 1 300\nwdens 5 4 0 0 0\ndens 1000 4096 1 0 300\n"
    got = [[int(v) for v in line.split()] for line in subprocess.run([TABLE], input=ask, capture_output=True, text=True,
                                                                     check=True).stdout.splitlines()]
    pop, src, count, temp, pts, ws, nodes, dens, row, part, temp_bytes, need = got[0]
    a = lambda b: (b + 255) & ~255   # noqa: E731
    assert (pop, src, count, temp, temp_bytes) == (0, 1024, a(1024 + 4000), a(a(1024 + 4000) + 8), 512)
    assert pts == temp + 512 and ws == a(pts + 16000) and nodes == a(ws + 8000) and dens == a(nodes + 16 * 4096)
    assert row == a(dens + 8 * 4096) and part == a(row + 8000) and need == part + 8 * (1024 * 1024 + 4096)
    assert got[1][9] == got[1][8] and got[1][11] < need          # the caller keeps the row: an empty piece
    assert got[2][11] == got[2][9] + 8 * (1024 * 1024 + 4)       # no sample pass: the nodes size the partial sums
    assert all(v % 256 == 0 for v in got[0][:10])
    # erpl_mc_impact_density's row: the same pieces without the weights
    assert got[3][:5] == [pop, src, count, temp, pts] and got[3][5] == a(pts + 16000) and len(got[3]) == 11


def test_engine_method_refuses_on_the_host():
    """No CPU path behind TrajectoryEngine.impact_density_weighted: the refusals come before the library is called (the engine
    here has no library and no context)."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.impact_density_weighted(eng, torch.zeros((16, 4), dtype=torch.float64), torch.zeros(4, dtype=torch.int64))
