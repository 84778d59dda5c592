"""erpl_mc_corridor_bands_weighted_defaults / erpl_mc_corridor_bands_weighted / _host at the C boundary, as far as it goes
without a GPU: the declarations, the structs and the constants against gcc, the defaults, every argument check in the order the
header states (they come before any device work and look at the context last, so a NULL context and dummy pointers that are never
dereferenced show them all), the host-side refusals of the engine method, of the analysis functions and of the analyzer - the
unknown `design` of a captured run among them - and the host rules through erpl_bands_w_check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
NAMES = ("erpl_mc_corridor_bands_weighted_defaults", "erpl_mc_corridor_bands_weighted", "erpl_mc_corridor_bands_weighted_host")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_symbols_are_declared_listed_documented_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)
    assert _abi.ABI_VERSION == 4 and lib.erpl_mc_abi_version() == 4


def test_structs_and_constants_match_the_c_compiler(tmp_path):
    macros = (("ERPL_BANDS_W_MAX_THRESHOLDS", _abi.BANDS_W_MAX_THRESHOLDS), ("ERPL_RW_MAX_Q", _abi.RW_MAX_Q),
              ("ERPL_CORRIDOR_MAX_CHANNELS", _abi.CORRIDOR_MAX_CHANNELS), ("ERPL_CORRIDOR_MAX_NODES", _abi.CORRIDOR_MAX_NODES))
    H.check_struct_layouts(tmp_path, (("erpl_bands_w_spec", "ErplBandsWSpec"), ("erpl_bands_w_row", "ErplBandsWRow"),
                                      ("erpl_bands_w_result", "ErplBandsWResult")), macros)
    # analysis.bands_weighted_result_dict reads an array of erpl_bands_w_row as 28 eight-byte words per record
    R = _abi.ErplBandsWRow
    assert C.sizeof(R) == 224 and R.exceed_w.offset == 32 and R.quantile.offset == 64 and R.min.offset == 128 and R.a2.offset == 192


def test_defaults(lib):
    s = _abi.ErplBandsWSpec()
    C.memset(C.byref(s), 0xff, C.sizeof(s))
    assert lib.erpl_mc_corridor_bands_weighted_defaults(C.byref(s)) == 0
    assert (s.n_channels, s.n_nodes, s.n_q, s.reserved) == (0, 0, 5, 0) and list(s.q) == [0.05, 0.25, 0.5, 0.75, 0.95, 0.0, 0.0, 0.0]
    assert not any(s.n_thresholds) and not any(v for row in s.threshold for v in row)
    assert lib.erpl_mc_corridor_bands_weighted_defaults(None) == -1 and "spec" in lib.erpl_mc_last_error().decode()


@pytest.mark.parametrize("host", (False, True))
def test_checks_come_before_any_device_work_in_the_stated_order(lib, host):
    D, N = H.DUMMY, None
    nan = float("nan")

    def spec(n_channels=2, n_nodes=5, n_q=1, q0=0.5, n_thr=(0, 0), thr=None):
        s = _abi.ErplBandsWSpec()
        s.n_channels, s.n_nodes, s.n_q = n_channels, n_nodes, n_q
        s.q[0] = q0
        s.n_thresholds[0], s.n_thresholds[1] = n_thr
        if thr is not None:
            s.threshold[thr[0]][thr[1]] = nan
        return s

    def call(s, values=D, weights=D, rows=D, result=True, m=5, ld=5):
        res = _abi.ErplBandsWResult()
        args = (values, N, weights, m, ld, C.byref(s) if s is not None else None, rows, C.byref(res) if result else None)
        rc = lib.erpl_mc_corridor_bands_weighted_host(*args) if host else lib.erpl_mc_corridor_bands_weighted(None, *args, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(word, *a, **kw):
        rc, msg = call(*a, **kw)
        assert rc == -1 and word in msg, (word, msg)

    # 1. a NULL spec, whatever else is wrong
    refused("spec", None, N, N, N, False, 0, -1)
    # 2. the spec, field by field, with everything behind it wrong too
    rest = dict(values=N, weights=N, rows=N, result=False, m=0, ld=-1)
    for c in (0, -1, 9):
        refused("n_channels", spec(c, 0, 9, 2.0, (5, 5)), **rest)
    for t in (0, -1, _abi.CORRIDOR_MAX_NODES + 1):
        refused("n_nodes", spec(2, t, 9, 2.0, (5, 5)), **rest)
    for n_q in (-1, 9):
        refused("n_q", spec(2, 5, n_q, 2.0, (5, 5)), **rest)
    for q in (-0.1, 1.5, nan):
        refused("q[0]", spec(2, 5, 1, q, (5, 5)), **rest)
    refused("n_thresholds[0]", spec(n_thr=(5, -1), thr=(1, 0)), **rest)
    refused("n_thresholds[1]", spec(n_thr=(4, -1), thr=(0, 0)), **rest)
    refused("threshold[1][2]", spec(n_thr=(0, 3), thr=(1, 2)), **rest)
    ok = spec(n_thr=(0, 2), thr=(1, 2))   # a NaN behind the thresholds in use is not looked at
    # 3. the pointers: values, weights, then the result pointers
    refused("values", ok, N, N, N, False, 0, -1)
    refused("weights", ok, D, N, N, False, 0, -1)
    refused("rows", ok, D, D, N, False, 0, -1)
    refused("result", ok, D, D, D, False, 0, -1)
    # 4. m, 5. ld
    for m in (0, -3, 1 << 31, 1 << 40):
        refused(f"m = {m}", ok, m=m, ld=-1)
    refused("ld = 4", ok, m=5, ld=4)
    # 6. only the context is left (the host twin has none: nothing to show there without reading memory)
    if not host:
        refused("ctx", ok)
        refused("ctx", spec(8, _abi.CORRIDOR_MAX_NODES, 8, 1.0, (4, 4)), m=(1 << 31) - 1, ld=1 << 40)
        refused("ctx", spec(1, 1, 0, 7.0, (0, 9)), m=1, ld=1)   # q and the thresholds of channels not in use are not looked at


def test_engine_and_analysis_refuse_on_the_host():
    """No CPU path behind the device call: the refusals are on the host, before the library is called (the engine here has no
    library and no context)."""
    import torch
    from erpl_monte_carlo_sim_amd import analysis
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    w = torch.ones(8, dtype=torch.int64)
    for bad in (torch.zeros((2, 4, 8), dtype=torch.float64), torch.zeros((2, 4, 8), dtype=torch.float32), None,
                torch.zeros((4, 8), dtype=torch.float64)):
        with pytest.raises(ValueError, match="values"):
            TrajectoryEngine.corridor_bands_weighted(eng, bad, w)
    with pytest.raises(ValueError, match="values"):
        analysis.reweighted_corridor(torch.zeros((4, 8), dtype=torch.float64), 0.0, 1.0, ["z"], None, [], [], engine=eng)
    with pytest.raises(ValueError, match="channels"):
        analysis.reweighted_corridor(torch.zeros((2, 4, 8), dtype=torch.float64), 0.0, 1.0, ["z"], None, [], [], engine=eng)
    # the spec and the host twin
    for kw, word in ((dict(quantiles=[0.5] * 9), "quantiles"), (dict(thresholds=[[1.0] * 5]), "thresholds"),
                     (dict(thresholds={3: [1.0]}), "channel 3")):
        with pytest.raises(ValueError, match=word):
            analysis.bands_weighted_spec(2, 5, **kw)
    with pytest.raises(ValueError, match="channels"):
        analysis.bands_weighted_spec(9, 5)
    with pytest.raises(ValueError, match="nodes"):
        analysis.bands_weighted_spec(2, 0)
    v = np.zeros((1, 2, 8))
    with pytest.raises(ValueError, match="values"):
        analysis.bands_weighted_host(v.astype(np.float32), np.ones(8, dtype=np.int64))
    with pytest.raises(ValueError, match="m = 9"):
        analysis.bands_weighted_host(v, np.ones(9, dtype=np.int64), m=9)
    with pytest.raises(ValueError, match="weights"):
        analysis.bands_weighted_host(v, np.ones(7, dtype=np.int64))
    with pytest.raises(ValueError, match="mask"):
        analysis.bands_weighted_host(v, np.ones(8, dtype=np.int64), mask=np.zeros(7, dtype=np.uint8))


def test_analyzer_refuses_an_unknown_design_and_a_run_without_one():
    """Both before an engine is created: no GPU is touched."""
    from erpl_monte_carlo_sim_amd import models
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    ic = dict(H.EXAMPLE_IC)
    for fly in (lambda: mc.flight_envelope(ic, 8, design="sobol"), lambda: mc.trajectory_corridor(ic, 8, design="sobol"),
                lambda: mc.impact_point_trace(ic, 8, design="sobol"),
                lambda: mc.debris_footprint(ic, 8, [(100.0, 5.0)], design="sobol")):
        with pytest.raises(ValueError, match="design: None or one of"):
            fly()
    with pytest.raises(ValueError, match="design"):
        mc.reweighted_corridor({"values": None, "summary": None, "time": [0.0, 1.0], "channels": ["z"], "reasons": None},
                               uncertainty={"mass_uncertainty": 0.01})


def test_host_rules_check_runs_clean(lib):
    exe = os.path.join(CSRC, "erpl_bands_w_check")
    assert os.path.exists(exe), "make all builds it"
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
