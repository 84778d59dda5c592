"""erpl_mc_corridor_depth_defaults / erpl_mc_corridor_depth at the C boundary, as far as it goes without a GPU: the
declarations, the structs and the constants against gcc, the defaults, every argument check in the order the header states
(they come before any device work and look at the context last, so a NULL context and dummy pointers that are never
dereferenced show them all), the host-side refusals of the engine method and the host rules through erpl_depth_check."""
import ctypes as C
import os
import subprocess

import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
NAMES = ("erpl_mc_corridor_depth_defaults", "erpl_mc_corridor_depth")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_symbols_are_declared_listed_documented_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def test_structs_and_constants_match_the_c_compiler(tmp_path):
    macros = (("ERPL_DEPTH_MAX_CHANNELS", _abi.DEPTH_MAX_CHANNELS), ("ERPL_DEPTH_MAX_NODES", _abi.DEPTH_MAX_NODES),
              ("ERPL_DEPTH_LDS_MAX", _abi.DEPTH_LDS_MAX), ("ERPL_CORRIDOR_MAX_CHANNELS", _abi.DEPTH_MAX_CHANNELS),
              ("ERPL_CORRIDOR_MAX_NODES", _abi.DEPTH_MAX_NODES))
    H.check_struct_layouts(tmp_path, (("erpl_depth_spec", "ErplDepthSpec"), ("erpl_depth_row", "ErplDepthRow"),
                                      ("erpl_depth_result", "ErplDepthResult")), macros)
    assert _abi.ABI_VERSION == 4
    # the engine reads an array of erpl_depth_row as 8 eight-byte words per record
    assert C.sizeof(_abi.ErplDepthRow) == 64 and _abi.ErplDepthRow.central_lo.offset == 16 and _abi.ErplDepthRow.whisker_hi.offset == 56
    assert C.sizeof(_abi.ErplDepthSpec) == 32


def test_defaults(lib):
    s = _abi.ErplDepthSpec()
    C.memset(C.byref(s), 0xff, C.sizeof(s))
    assert lib.erpl_mc_corridor_depth_defaults(C.byref(s)) == 0
    assert (s.n_channels, s.n_nodes, s.central, s.factor, s.lds_limit, s.reserved) == (0, 0, 0.5, 1.5, 0, 0)
    assert lib.erpl_mc_corridor_depth_defaults(None) == -1 and "spec" in lib.erpl_mc_last_error().decode()


def test_checks_come_before_any_device_work_in_the_stated_order(lib):
    D = H.DUMMY
    nan, inf = float("nan"), float("inf")

    def spec(n_channels=3, n_nodes=7, central=0.5, factor=1.5, lds_limit=0):
        s = _abi.ErplDepthSpec()
        s.n_channels, s.n_nodes, s.central, s.factor, s.lds_limit = n_channels, n_nodes, central, factor, lds_limit
        return s

    def call(s, values=D, ld=5, m=5, result=True, rows=D, depth=D, mei=D, nodes=D, n_out=D, first_out=D, central=D):
        res = _abi.ErplDepthResult()
        rc = lib.erpl_mc_corridor_depth(None, values, ld, None, m, C.byref(s) if s is not None else None,
                                        C.byref(res) if result else None, rows, depth, mei, nodes, n_out, first_out, central, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(word, *a, **kw):
        rc, msg = call(*a, **kw)
        assert rc == -1 and word in msg, (word, msg)

    bad = spec(0, 0, 0.0, -1.0, -1)   # every field wrong: what is checked before the fields is still named first
    # 1. the pointers, in the order spec, values, result, rows, depth, mei, nodes, n_out, first_out, central
    N = None
    refused("spec", None, N, -1, 0, False, N, N, N, N, N, N, N)
    refused("values", bad, N, -1, 0, False, N, N, N, N, N, N, N)
    refused("result", bad, D, -1, 0, False, N, N, N, N, N, N, N)
    refused("rows", bad, D, -1, 0, True, N, N, N, N, N, N, N)
    refused("depth", bad, D, -1, 0, True, D, N, N, N, N, N, N)
    refused("mei", bad, D, -1, 0, True, D, D, N, N, N, N, N)
    refused("nodes", bad, D, -1, 0, True, D, D, D, N, N, N, N)
    refused("n_out", bad, D, -1, 0, True, D, D, D, D, N, N, N)
    refused("first_out", bad, D, -1, 0, True, D, D, D, D, D, N, N)
    refused("central is NULL", bad, D, -1, 0, True, D, D, D, D, D, D, N)
    # 2. m, then ld
    for m in (0, -3, 1 << 31, 1 << 40):
        refused(f"m = {m}", bad, ld=-1, m=m)
    refused("ld = 4", bad, ld=4, m=5)
    # 3. the spec: n_channels, n_nodes, central, factor, lds_limit
    for c in (0, -1, 9):
        refused("n_channels", spec(c, 0, 0.0, -1.0, -1))
    for t in (0, -1, _abi.DEPTH_MAX_NODES + 1):
        refused("n_nodes", spec(3, t, 0.0, -1.0, -1))
    for v in (0.0, -1.0, 1.5, nan):
        refused("spec->central", spec(3, 7, v, -1.0, -1))
    for v in (-1.0, inf, nan):
        refused("spec->factor", spec(3, 7, 1.0, v, -1))
    for v in (-1, -(1 << 31)):
        refused("lds_limit", spec(3, 7, 1.0, 0.0, v))
    # 4. only the context is left
    refused("ctx", spec())
    refused("ctx", spec(8, _abi.DEPTH_MAX_NODES, 1.0, 0.0, (1 << 31) - 1), ld=1 << 40, m=(1 << 31) - 1)
    refused("ctx", spec(1, 1, 5e-324, 1e308, 1), ld=1, m=1)


def test_engine_method_refuses_host_tensors_and_wrong_dtypes():
    """No CPU path behind the call: the refusals are on the host, before the library is called (the engine here has no
    library and no context)."""
    import torch
    from erpl_monte_carlo_sim_amd import analysis
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    for bad in (torch.zeros((2, 4, 8), dtype=torch.float64), torch.zeros((2, 4, 8), dtype=torch.float32), None,
                torch.zeros((4, 8), dtype=torch.float64)):
        with pytest.raises(ValueError, match="values"):
            TrajectoryEngine.corridor_depth(eng, bad)
    with pytest.raises(ValueError, match="values"):
        analysis.trajectory_depth(torch.zeros((4, 8), dtype=torch.float64), engine=eng)
    with pytest.raises(ValueError, match="channels"):
        analysis.trajectory_depth(torch.zeros((2, 4, 8), dtype=torch.float64), channels=["z"], engine=eng)


def test_host_rules_check_runs_clean(lib):
    exe = os.path.join(CSRC, "erpl_depth_check")
    assert os.path.exists(exe), "make all builds it"
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok erpl_depth_check"), out.stdout + out.stderr
