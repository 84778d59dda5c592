"""erpl_mc_analysis_defaults / erpl_mc_analyze at the C boundary, as far as it goes without a GPU: struct layouts,
the default bounds, and the argument checks (which come before any device work and look at the context last)."""
import ctypes as C
import os

import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = (("erpl_analysis_spec", "ErplAnalysisSpec"), ("erpl_row_stats", "ErplRowStats"), ("erpl_analysis", "ErplAnalysis"))
MACROS = (("ERPL_ANALYSIS_MAX_ROWS", _abi.ANALYSIS_MAX_ROWS), ("ERPL_ANALYSIS_MAX_Q", _abi.ANALYSIS_MAX_Q))


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def defaults(lib):
    spec = _abi.ErplAnalysisSpec()
    assert lib.erpl_mc_analysis_defaults(C.byref(spec)) == 0
    return spec


def test_analysis_struct_layout_matches_c_compiler(tmp_path):
    """sizeof and the offset of every field of the three ctypes mirrors == what gcc sees in include/erpl_mc.h."""
    H.check_struct_layouts(tmp_path, STRUCTS, MACROS)


def test_reason_bits_match_the_header():
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    for name, val in (("NON_FINITE", _abi.WHY_NON_FINITE), ("APOGEE_HIGH", _abi.WHY_APOGEE_HIGH),
                      ("APOGEE_LOW", _abi.WHY_APOGEE_LOW), ("RANGE", _abi.WHY_RANGE),
                      ("FLIGHT_TIME", _abi.WHY_FLIGHT_TIME), ("ENERGY", _abi.WHY_ENERGY)):
        assert f"ERPL_WHY_{name} = {val}" in hdr, name
    assert [1 << k for k in range(6)] == [_abi.WHY_NON_FINITE, _abi.WHY_APOGEE_HIGH, _abi.WHY_APOGEE_LOW, _abi.WHY_RANGE,
                                          _abi.WHY_FLIGHT_TIME, _abi.WHY_ENERGY]
    assert len(_abi.WHY_NAMES) == 6 and len(_abi.END_NAMES) == 5


def test_defaults_are_the_pinned_host_bounds(lib):
    """Needs no GPU and no context.  Equality is exact: the energy bound is evaluated in the reference's order."""
    spec = defaults(lib)
    assert spec.max_apogee == analysis.MAX_REASONABLE_APOGEE
    assert spec.min_apogee == analysis.MIN_REASONABLE_APOGEE
    assert spec.max_range == analysis.MAX_REASONABLE_RANGE
    assert spec.max_flight_time == analysis.MAX_REASONABLE_FLIGHT_TIME
    assert spec.energy_apogee == analysis._THEORETICAL_MAX_ALTITUDE * 1.2
    assert spec.n_rows == 3 and list(spec.rows[:3]) == [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
    assert spec.n_q == 5 and list(spec.q[:5]) == [0.05, 0.25, 0.5, 0.75, 0.95]
    assert lib.erpl_mc_analysis_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_argument_checks_come_before_any_device_work(lib):
    """spec, n and the pointers are checked before the context, so every refusal can be seen without a device: a
    non-NULL dummy that is never dereferenced stands in for the summary, and the context is NULL throughout."""
    dummy = H.DUMMY
    res = _abi.ErplAnalysis()

    def call(spec, n=8, summary=dummy, result=res):
        rc = lib.erpl_mc_analyze(None, summary, None, n, C.byref(spec) if spec is not None else None,
                                 C.byref(result) if result is not None else None, None, None)
        return rc, lib.erpl_mc_last_error().decode()

    rc, msg = call(None)
    assert rc == -1 and "spec" in msg
    rc, msg = call(defaults(lib), n=0)
    assert rc == -1 and "n = 0" in msg
    rc, msg = call(defaults(lib), n=-5)
    assert rc == -1 and "n = -5" in msg
    spec = defaults(lib)
    spec.rows[2] = spec.rows[0]
    rc, msg = call(spec)
    assert rc == -1 and "rows[2]" in msg and "twice" in msg
    spec = defaults(lib)
    spec.rows[1] = 16
    rc, msg = call(spec)
    assert rc == -1 and "rows[1]" in msg and "16" in msg
    spec = defaults(lib)
    spec.rows[0] = -1
    assert call(spec)[0] == -1
    spec = defaults(lib)
    spec.q[3] = 1.5
    rc, msg = call(spec)
    assert rc == -1 and "q[3]" in msg
    spec = defaults(lib)
    spec.q[0] = float("nan")
    rc, msg = call(spec)
    assert rc == -1 and "q[0]" in msg
    spec = defaults(lib)
    spec.max_range = float("nan")
    rc, msg = call(spec)
    assert rc == -1 and "max_range" in msg
    for field, bad in (("n_rows", 17), ("n_rows", -1), ("n_q", 9), ("n_q", -1)):
        spec = defaults(lib)
        setattr(spec, field, bad)
        rc, msg = call(spec)
        assert rc == -1 and field in msg, field
    rc, msg = call(defaults(lib), summary=None)
    assert rc == -1 and "summary" in msg
    rc, msg = call(defaults(lib), result=None)
    assert rc == -1 and "result" in msg
    # everything else in order: only the context is left to refuse
    rc, msg = call(defaults(lib))
    assert rc == -1 and "ctx" in msg


def test_engine_analyze_refuses_host_tensors():
    """There is no CPU path behind TrajectoryEngine.analyze: the check is on the host, before the library is called."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)       # no context: the refusal must come first
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.analyze(eng, torch.zeros((16, 4), dtype=torch.float64))
