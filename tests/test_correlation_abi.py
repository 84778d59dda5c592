"""erpl_mc_correlation and its defaults function at the C boundary, as far as it goes without a GPU: struct layouts against
gcc, the defaults, every argument check (they come before any device work and look at the context last, so a NULL context
and a dummy pointer that is never dereferenced show them all), and the host helpers of analysis.drivers."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = H.DUMMY

STRUCTS = (("erpl_corr_spec", "ErplCorrSpec"), ("erpl_corr_result", "ErplCorrResult"))
MACROS = (("ERPL_CORR_MAX_FACTORS", _abi.CORR_MAX_FACTORS), ("ERPL_CORR_MAX_ROWS", _abi.CORR_MAX_ROWS),
          ("ERPL_CORR_MAX_VARS", _abi.CORR_MAX_VARS))


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and the offset of EVERY field of the two ctypes mirrors == what gcc sees in include/erpl_mc.h."""
    H.check_struct_layouts(tmp_path, STRUCTS, MACROS)
    assert (_abi.CORR_MAX_FACTORS, _abi.CORR_MAX_ROWS, _abi.CORR_MAX_VARS) == (32, 16, 48)
    assert _abi.CORR_MAX_ROWS == _abi.SUMMARY_DIM and _abi.ABI_VERSION == 4


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_correlation_defaults", "erpl_mc_correlation"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def defaults(lib, n_factors=3):
    spec = _abi.ErplCorrSpec()
    assert lib.erpl_mc_correlation_defaults(C.byref(spec)) == 0
    spec.n_factors = n_factors
    return spec


def test_defaults(lib):
    spec = _abi.ErplCorrSpec()
    spec.n_factors, spec.reserved = 7, 9
    assert lib.erpl_mc_correlation_defaults(C.byref(spec)) == 0
    assert spec.n_factors == 0 and spec.reserved == 0 and spec.ranks == 1
    assert spec.n_rows == 3 and list(spec.rows[:3]) == [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
    assert lib.erpl_mc_correlation_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_argument_checks_come_before_any_device_work(lib):
    res = _abi.ErplCorrResult()

    def call(spec, n=8, factors=DUMMY, summary=DUMMY, result=res, corr=None, rank_corr=None, ranks_out=None):
        rc = lib.erpl_mc_correlation(None, factors, summary, None, n, C.byref(spec) if spec is not None else None,
                                     C.byref(result) if result is not None else None, corr, rank_corr, ranks_out, None)
        return rc, lib.erpl_mc_last_error().decode()

    rc, msg = call(None)
    assert rc == -1 and "spec" in msg
    for n in (0, -5):
        rc, msg = call(defaults(lib), n=n)
        assert rc == -1 and f"n = {n}" in msg
    for bad in (0, 33, -1):
        rc, msg = call(defaults(lib, n_factors=bad))
        assert rc == -1 and "n_factors" in msg and str(bad) in msg
    for bad in (0, 17, -1):
        spec = defaults(lib)
        spec.n_rows = bad
        rc, msg = call(spec)
        assert rc == -1 and "n_rows" in msg and str(bad) in msg
    spec = defaults(lib)
    spec.rows[2] = spec.rows[0]
    rc, msg = call(spec)
    assert rc == -1 and "rows[2]" in msg and "twice" in msg
    for bad in (16, -1):
        spec = defaults(lib)
        spec.rows[1] = bad
        rc, msg = call(spec)
        assert rc == -1 and "rows[1]" in msg and str(bad) in msg
    for bad in (2, -1):
        spec = defaults(lib)
        spec.ranks = bad
        rc, msg = call(spec)
        assert rc == -1 and "ranks" in msg and str(bad) in msg
    # ranks = 0: there is nothing to put into rank_corr / ranks_out
    spec = defaults(lib)
    spec.ranks = 0
    rc, msg = call(spec, rank_corr=DUMMY)
    assert rc == -1 and "rank_corr" in msg
    rc, msg = call(spec, ranks_out=DUMMY)
    assert rc == -1 and "ranks_out" in msg
    for name in ("factors", "summary"):
        rc, msg = call(defaults(lib), **{name: None})
        assert rc == -1 and name in msg
    rc, msg = call(defaults(lib), result=None)
    assert rc == -1 and "result" in msg
    # everything in order, at the limits: only the context is left
    spec = defaults(lib, n_factors=32)
    spec.n_rows = 16
    spec.rows[:16] = list(range(15, -1, -1))
    rc, msg = call(spec, corr=DUMMY, rank_corr=DUMMY, ranks_out=DUMMY)
    assert rc == -1 and "ctx" in msg
    spec = defaults(lib, n_factors=1)
    spec.n_rows, spec.ranks = 1, 0
    rc, msg = call(spec, corr=DUMMY)
    assert rc == -1 and "ctx" in msg


def test_engine_correlation_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.correlation: the refusal is on the host, before the library is called."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.correlation(eng, torch.zeros((2, 4), dtype=torch.float64), torch.zeros((16, 4), dtype=torch.float64))


def test_factors_from_results_flattens_the_parameter_dicts():
    def rec(i, motor=True, **extra):
        p = {"initial_position_offset": np.array([0.0, 0.0, 0.0]), "initial_velocity_offset": np.array([0.1 * i, 0.2, 0.3]),
             "initial_attitude_offset": [0.01, 0.02 * i, 0.03], "initial_angular_velocity_offset": np.array([1.0, 2.0, 3.0 + i]),
             "mass_multiplier": 1.0 + 0.01 * i, "thrust_multiplier": 0.97, "wind_speed": 2.5 * i, "wind_direction": 0.5,
             "density_multiplier": 1.02, "random_seed": i}
        r = {"apogee_altitude": 9000.0 + i, "range": 100.0 * i, "flight_time": 60.0, "simulation_id": i, "parameters": p}
        if motor:
            r["motor_inputs"] = {"motor_thrust": 13000.0 + i, "motor_mass_flow_rate": 4.0 + 0.1 * i}
        r.update(extra)
        return r

    fac, names = analysis.factors_from_results([rec(0), None, rec(1), rec(2)])
    assert names == ([f"{k}[{c}]" for k in ("initial_position_offset", "initial_velocity_offset", "initial_attitude_offset",
                                            "initial_angular_velocity_offset") for c in range(3)]
                     + ["mass_multiplier", "thrust_multiplier", "wind_speed", "wind_direction", "density_multiplier",
                        "motor_thrust", "motor_mass_flow_rate"])
    assert "random_seed" not in names
    assert fac.shape == (19, 3) and fac.dtype == np.float64
    col = dict(zip(names, fac))
    assert col["initial_velocity_offset[0]"].tolist() == [0.0, 0.1, 0.2]
    assert col["initial_attitude_offset[1]"].tolist() == [0.0, 0.02, 0.04]
    assert col["initial_angular_velocity_offset[2]"].tolist() == [3.0, 4.0, 5.0]
    assert col["mass_multiplier"].tolist() == [1.0, 1.01, 1.02]
    assert col["thrust_multiplier"].tolist() == [0.97] * 3 and col["density_multiplier"].tolist() == [1.02] * 3
    assert col["wind_speed"].tolist() == [0.0, 2.5, 5.0]
    assert col["motor_thrust"].tolist() == [13000.0, 13001.0, 13002.0]
    assert col["motor_mass_flow_rate"].tolist() == [4.0, 4.1, 4.2]
    # the reference's own records carry no motor inputs: 17 rows
    fac, names = analysis.factors_from_results([rec(0, motor=False), rec(3, motor=False)])
    assert fac.shape == (17, 2) and names[-1] == "density_multiplier"
    # a record without one of the keys: NaN there, so that listwise deletion drops it
    broken = rec(5)
    del broken["parameters"]["wind_speed"]
    fac, names = analysis.factors_from_results([rec(0), broken])
    assert np.isnan(fac[names.index("wind_speed"), 1]) and fac[names.index("wind_speed"), 0] == 0.0
    summ = analysis.summary_from_results([rec(0), rec(4, impact_position=[1.0, 2.0, 0.0])])
    assert summ.shape == (16, 2) and summ[_abi.SUM_RANGE].tolist() == [0.0, 400.0]
    assert summ[_abi.SUM_IMPACT_Y, 1] == 2.0 and np.isnan(summ[_abi.SUM_IMPACT_Y, 0])


def test_ranking_orders_by_magnitude_with_constant_factors_last():
    nan = float("nan")
    names = ["a", "b", "c", "d", "e"]
    corr = {"spearman": np.array([[0.1, -0.9, nan, 0.5, -0.5], [nan, nan, 0.0, -0.2, 0.3]]),
            "pearson": np.array([[-0.7, 0.2, nan, 0.1, 0.0], [nan, nan, 0.4, 0.9, -0.1]])}
    assert analysis.rank_drivers(corr, names) == [["b", "d", "e", "a", "c"], ["e", "d", "c", "a", "b"]]
    assert analysis.rank_drivers(corr, names, ranks=False) == [["a", "b", "d", "e", "c"], ["d", "c", "e", "a", "b"]]
