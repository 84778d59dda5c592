"""erpl_mc_histogram / erpl_mc_histogram_xy / erpl_mc_dispersion and their two defaults functions at the C boundary, as far
as it goes without a GPU: struct layouts against gcc, the defaults, and every argument check (they come before any device
work and look at the context last, so a NULL context and a dummy pointer that is never dereferenced show them all)."""
import ctypes as C
import math
import os

import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
DUMMY = H.DUMMY

STRUCTS = (("erpl_hist_spec", "ErplHistSpec"), ("erpl_hist_result", "ErplHistResult"),
           ("erpl_hist2d_spec", "ErplHist2dSpec"), ("erpl_hist2d_result", "ErplHist2dResult"),
           ("erpl_dispersion_spec", "ErplDispersionSpec"), ("erpl_dispersion", "ErplDispersion"))
MACROS = (("ERPL_HIST_MAX_ROWS", _abi.HIST_MAX_ROWS), ("ERPL_HIST_MAX_BINS", _abi.HIST_MAX_BINS),
          ("ERPL_HIST2D_MAX_BINS", _abi.HIST2D_MAX_BINS), ("ERPL_DISP_MAX_LEVELS", _abi.DISP_MAX_LEVELS),
          ("ERPL_CENTRE_MEAN", _abi.CENTRE_MEAN), ("ERPL_CENTRE_POINT", _abi.CENTRE_POINT))


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and the offset of EVERY field of the six new ctypes mirrors == what gcc sees in include/erpl_mc.h."""
    H.check_struct_layouts(tmp_path, STRUCTS, MACROS)
    assert _abi.ABI_VERSION == 4


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_histogram_defaults", "erpl_mc_histogram", "erpl_mc_histogram_xy", "erpl_mc_dispersion_defaults",
                 "erpl_mc_dispersion"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def hist_defaults(lib):
    spec = _abi.ErplHistSpec()
    assert lib.erpl_mc_histogram_defaults(C.byref(spec)) == 0
    return spec


def disp_defaults(lib):
    spec = _abi.ErplDispersionSpec()
    assert lib.erpl_mc_dispersion_defaults(C.byref(spec)) == 0
    return spec


def test_defaults(lib):
    spec = hist_defaults(lib)
    assert spec.n_rows == 3 and list(spec.rows[:3]) == [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
    assert list(spec.bins[:3]) == [50, 50, 50]
    assert all(math.isnan(spec.lo[j]) and math.isnan(spec.hi[j]) for j in range(3))
    assert lib.erpl_mc_histogram_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()
    d = disp_defaults(lib)
    assert (d.row_x, d.row_y) == (_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y)
    assert d.centre == _abi.CENTRE_POINT and d.cx == 0.0 and d.cy == 0.0
    assert d.n_levels == 3 and list(d.level[:3]) == [0.5, 0.9, 0.99]
    assert d.n_q == 4 and list(d.q[:4]) == [0.5, 0.9, 0.95, 0.99]
    assert lib.erpl_mc_dispersion_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_histogram_argument_checks_come_before_any_device_work(lib):
    res = _abi.ErplHistResult()

    def call(spec, n=8, summary=DUMMY, edges=DUMMY, counts=DUMMY, result=res):
        rc = lib.erpl_mc_histogram(None, summary, None, n, C.byref(spec) if spec is not None else None, edges, counts,
                                   C.byref(result) if result is not None else None, None)
        return rc, lib.erpl_mc_last_error().decode()

    rc, msg = call(None)
    assert rc == -1 and "spec" in msg
    for n in (0, -5):
        rc, msg = call(hist_defaults(lib), n=n)
        assert rc == -1 and f"n = {n}" in msg
    for bad in (0, 17, -1):
        spec = hist_defaults(lib)
        spec.n_rows = bad
        rc, msg = call(spec)
        assert rc == -1 and "n_rows" in msg
    spec = hist_defaults(lib)
    spec.rows[2] = spec.rows[0]
    rc, msg = call(spec)
    assert rc == -1 and "rows[2]" in msg and "twice" in msg
    for bad in (16, -1):
        spec = hist_defaults(lib)
        spec.rows[1] = bad
        rc, msg = call(spec)
        assert rc == -1 and "rows[1]" in msg and str(bad) in msg
    for bad in (0, 1025, -3):
        spec = hist_defaults(lib)
        spec.bins[1] = bad
        rc, msg = call(spec)
        assert rc == -1 and "bins[1]" in msg and str(bad) in msg
    spec = hist_defaults(lib)
    spec.lo[0], spec.hi[0] = 2.0, 1.0
    rc, msg = call(spec)
    assert rc == -1 and "lo[0]" in msg and "hi[0]" in msg
    for lo, hi in ((NAN, 1.0), (1.0, NAN), (-math.inf, 1.0), (0.0, math.inf), (-1e308, 1e308)):
        spec = hist_defaults(lib)
        spec.lo[2], spec.hi[2] = lo, hi
        rc, msg = call(spec)
        assert rc == -1 and "lo[2]" in msg and "hi[2]" in msg, (lo, hi)
    for name in ("summary", "edges", "counts"):
        rc, msg = call(hist_defaults(lib), **{name: None})
        assert rc == -1 and name in msg
    rc, msg = call(hist_defaults(lib), result=None)
    assert rc == -1 and "result" in msg
    # everything in order, explicit ranges included (lo == hi is allowed: np.histogram widens it): only the context is left
    spec = hist_defaults(lib)
    spec.lo[0], spec.hi[0] = 0.0, 1.0
    spec.lo[1], spec.hi[1] = 5.0, 5.0
    spec.bins[2] = 1024
    rc, msg = call(spec)
    assert rc == -1 and "ctx" in msg


def test_histogram2d_argument_checks_come_before_any_device_work(lib):
    res = _abi.ErplHist2dResult()

    def good():
        return _abi.ErplHist2dSpec(_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, 50, 256, NAN, NAN, 0.0, 1.0)

    def call(spec, n=8, summary=DUMMY, edges_x=DUMMY, edges_y=DUMMY, counts=DUMMY, result=res):
        rc = lib.erpl_mc_histogram_xy(None, summary, None, n, C.byref(spec) if spec is not None else None, edges_x, edges_y,
                                     counts, C.byref(result) if result is not None else None, None)
        return rc, lib.erpl_mc_last_error().decode()

    rc, msg = call(None)
    assert rc == -1 and "spec" in msg
    rc, msg = call(good(), n=0)
    assert rc == -1 and "n = 0" in msg
    for field, bad in (("row_x", 16), ("row_y", -1), ("bins_x", 0), ("bins_y", 257)):
        spec = good()
        setattr(spec, field, bad)
        rc, msg = call(spec)
        assert rc == -1 and field in msg and str(bad) in msg, field
    spec = good()
    spec.row_y = spec.row_x
    rc, msg = call(spec)
    assert rc == -1 and "twice" in msg
    spec = good()
    spec.lo_x, spec.hi_x = 1.0, 0.0
    rc, msg = call(spec)
    assert rc == -1 and "lo_x" in msg and "hi_x" in msg
    spec = good()
    spec.hi_y = NAN
    rc, msg = call(spec)
    assert rc == -1 and "lo_y" in msg and "hi_y" in msg
    for name in ("summary", "edges_x", "edges_y", "counts"):
        rc, msg = call(good(), **{name: None})
        assert rc == -1 and name in msg
    rc, msg = call(good(), result=None)
    assert rc == -1 and "result" in msg
    rc, msg = call(good())
    assert rc == -1 and "ctx" in msg


def test_dispersion_argument_checks_come_before_any_device_work(lib):
    res = _abi.ErplDispersion()

    def call(spec, n=8, summary=DUMMY, result=res):
        rc = lib.erpl_mc_dispersion(None, summary, None, n, C.byref(spec) if spec is not None else None,
                                    C.byref(result) if result is not None else None, None, None)
        return rc, lib.erpl_mc_last_error().decode()

    rc, msg = call(None)
    assert rc == -1 and "spec" in msg
    rc, msg = call(disp_defaults(lib), n=-1)
    assert rc == -1 and "n = -1" in msg
    for field, bad in (("row_x", 16), ("row_y", -1), ("centre", 2), ("n_levels", 9), ("n_levels", -1), ("n_q", 9), ("n_q", -1)):
        spec = disp_defaults(lib)
        setattr(spec, field, bad)
        rc, msg = call(spec)
        assert rc == -1 and field in msg, field
    spec = disp_defaults(lib)
    spec.row_y = spec.row_x
    rc, msg = call(spec)
    assert rc == -1 and "twice" in msg
    for bad in (0.0, 1.0, -0.1, 1.5, NAN):
        spec = disp_defaults(lib)
        spec.level[1] = bad
        rc, msg = call(spec)
        assert rc == -1 and "level[1]" in msg, bad
    for bad in (-0.01, 1.01, NAN):
        spec = disp_defaults(lib)
        spec.q[3] = bad
        rc, msg = call(spec)
        assert rc == -1 and "q[3]" in msg, bad
    spec = disp_defaults(lib)
    spec.cx = NAN
    rc, msg = call(spec)
    assert rc == -1 and "cx" in msg
    rc, msg = call(disp_defaults(lib), summary=None)
    assert rc == -1 and "summary" in msg
    rc, msg = call(disp_defaults(lib), result=None)
    assert rc == -1 and "result" in msg
    spec = disp_defaults(lib)
    spec.q[0], spec.q[1] = 0.0, 1.0          # the ends of [0, 1] are quantiles
    spec.centre = _abi.CENTRE_MEAN
    spec.cx = NAN                            # not looked at about the mean
    rc, msg = call(spec)
    assert rc == -1 and "ctx" in msg


def test_engine_methods_refuse_host_tensors():
    """No CPU path behind TrajectoryEngine.histogram / histogram2d / dispersion: the refusal is on the host, before the
    library is called (the engine here has no library and no context)."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    host = torch.zeros((16, 4), dtype=torch.float64)
    for method in (TrajectoryEngine.histogram, TrajectoryEngine.histogram2d, TrajectoryEngine.dispersion):
        with pytest.raises(ValueError, match="summary"):
            method(eng, host)
