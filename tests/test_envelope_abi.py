"""erpl_mc_flight_envelope at the C boundary, as far as it goes without a GPU: the declaration, the row constants against
gcc, every argument check in the order the header states (they come before any device work and look at the context last,
so a NULL context and dummy pointers that are never dereferenced show them all), the host-side refusal of the engine
method and the row names of the analysis layer."""
import ctypes as C
import os

import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = H.DUMMY.value

ROWS = ("MAX_Q", "MAX_Q_TIME", "MAX_Q_ALT", "MAX_Q_MACH", "MAX_MACH", "MAX_Q_ALPHA", "MAX_AXIAL_ACCEL", "MIN_STABILITY",
        "MAX_OMEGA", "MAX_QUAT_DEV", "BURNOUT_TIME", "BURNOUT_ALT", "BURNOUT_SPEED", "BURNOUT_STABILITY", "APOGEE_RECORD",
        "USABLE")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_symbol_is_declared_listed_documented_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    name = "erpl_mc_flight_envelope"
    assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc
    getattr(lib, name)


def test_row_constants_match_the_c_compiler(tmp_path):
    macros = (("ERPL_ENV_DIM", _abi.ENV_DIM),) + tuple(("ERPL_ENV_" + r, getattr(_abi, "ENV_" + r)) for r in ROWS)
    H.check_struct_layouts(tmp_path, (), macros)
    assert [getattr(_abi, "ENV_" + r) for r in ROWS] == list(range(16))
    assert _abi.ENV_DIM == _abi.SUMMARY_DIM == 16 and _abi.ABI_VERSION == 4


def good():
    """A batch and an out that pass every check: only the context is left."""
    b, o = _abi.ErplBatch(), _abi.ErplOut()
    b.n, b.precision, b.k_wind = 8, _abi.PREC_F64_FAST, 6
    b.rocket = b.motor = b.alt_grid = b.wind = DUMMY
    o.n_traj, o.traj_cap = 3, 100
    o.traj_ids = o.traj = o.traj_len = DUMMY
    return b, o


def test_argument_checks_come_before_any_device_work_in_the_stated_order(lib):
    def call(b, o, envelope=H.DUMMY):
        rc = lib.erpl_mc_flight_envelope(None, C.byref(b) if b is not None else None, C.byref(o) if o is not None else None,
                                         envelope, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(word, batch=(), out=(), **kw):
        """`word` names the refused argument although everything that is checked LATER is wrong too."""
        b, o = good()
        for k, v in batch:
            setattr(b, k, v)
        for k, v in out:
            setattr(o, k, v)
        rc, msg = call(b, o, **kw)
        assert rc == -1 and word in msg, (word, msg)

    # everything behind the argument under test is broken as well: the message shows which check came first
    later_out = [("traj_cap", 0), ("traj_ids", None), ("traj", None), ("traj_len", None)]
    later_batch = [("rocket", None), ("motor", None), ("k_wind", 2000)]
    # 1. the three pointers
    rc, msg = call(None, None, None)
    assert rc == -1 and "batch" in msg
    rc, msg = call(good()[0], None, None)
    assert rc == -1 and "out" in msg
    refused("envelope", batch=[("precision", _abi.PREC_F32)], envelope=None)
    # 2. the precision
    for bad in (_abi.PREC_F32, 3, -1):
        refused("precision", batch=[("precision", bad), ("n", 0)] + later_batch, out=[("n_traj", -1)] + later_out)
    # 3. the batch size
    for bad in (0, -5):
        refused(f"n = {bad}", batch=[("n", bad)] + later_batch, out=[("n_traj", -1)] + later_out)
    # 4. n_traj
    for bad in (-1, 1 << 31, 1 << 40):
        refused(f"n_traj = {bad}", batch=later_batch, out=[("n_traj", bad)] + later_out)
    # 5. with trajectories: the capture, then the batch's tables
    refused("traj_cap", batch=later_batch, out=later_out)
    refused("traj_ids", batch=later_batch, out=later_out[1:])
    refused("traj_len", batch=later_batch, out=later_out[3:])
    refused("traj", batch=later_batch, out=later_out[2:3])
    assert "traj_ids" not in lib.erpl_mc_last_error().decode() and "traj_len" not in lib.erpl_mc_last_error().decode()
    refused("rocket", batch=later_batch)
    refused("motor", batch=later_batch[1:])
    refused("wind", batch=later_batch[2:])
    refused("wind", batch=[("k_wind", -1)])
    refused("wind", batch=[("alt_grid", None)])
    refused("wind", batch=[("wind", None)])
    # 6. only the context is left: both fp64 precisions, no wind table, the largest n_traj
    for prec in (_abi.PREC_F64, _abi.PREC_F64_FAST):
        refused("ctx", batch=[("precision", prec)])
    refused("ctx", batch=[("k_wind", 0), ("alt_grid", None), ("wind", None)], out=[("n_traj", (1 << 31) - 1)])
    # without trajectories nothing of the capture or the tables is looked at; the context still is
    refused("ctx", batch=later_batch, out=[("n_traj", 0)] + later_out)


def test_engine_method_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.flight_envelope: the refusal is on the host, before the library is called (the
    engine here has no library and no context, and there is no batch)."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    ids, tlen = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="traj"):
        TrajectoryEngine.flight_envelope(eng, None, ids, torch.zeros((2, 4, 15), dtype=torch.float64), tlen)
    with pytest.raises(ValueError, match="traj"):
        TrajectoryEngine.flight_envelope(eng, None, ids, None, tlen)


def test_envelope_names():
    assert len(analysis.ENVELOPE_NAMES) == _abi.ENV_DIM == 16 and len(set(analysis.ENVELOPE_NAMES)) == 16
    assert all(isinstance(s, str) and s for s in analysis.ENVELOPE_NAMES)
    assert analysis.ENVELOPE_NAMES[_abi.ENV_MAX_Q] == "max_q" and analysis.ENVELOPE_NAMES[_abi.ENV_USABLE] == "usable_records"
