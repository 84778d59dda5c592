"""erpl_mc_impact_points at the C boundary, as far as it goes without a GPU: the declarations, the constants and the layout
of erpl_iip_spec against gcc, the defaults, every argument check in the order the header states (they come before any device
work and look at the context last, so a NULL context and dummy pointers that are never dereferenced show them all), the
host-side refusal of the engine method and the names of the analysis layer."""
import ctypes as C
import os

import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = H.DUMMY.value

ROWS = ("MAX_RANGE", "MAX_RANGE_TIME", "MAX_RANGE_X", "MAX_RANGE_Y", "BURNOUT_TIME", "BURNOUT_X", "BURNOUT_Y", "APOGEE_X",
        "APOGEE_Y", "MAX_RATE", "MAX_RATE_TIME", "EXIT_TIME", "EXIT_X", "EXIT_Y", "LANDED", "NODES")
CHANNELS = ("X", "Y", "RANGE", "TFALL", "VIMPACT")
NAMES = ("erpl_mc_impact_points_defaults", "erpl_mc_impact_points")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_symbols_are_declared_listed_documented_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc
        getattr(lib, name)


def test_constants_and_struct_layout_match_the_c_compiler(tmp_path):
    macros = (("ERPL_IIP_DIM", _abi.IIP_DIM), ("ERPL_IIP_MAX_NODES", _abi.IIP_MAX_NODES), ("ERPL_IIP_MAX_STEPS", _abi.IIP_MAX_STEPS),
              ("ERPL_IIP_MAX_VERTICES", _abi.IIP_MAX_VERTICES), ("ERPL_IIP_CH_COUNT", _abi.IIP_CH_COUNT))
    macros += tuple(("ERPL_IIP_" + r, getattr(_abi, "IIP_" + r)) for r in ROWS)
    macros += tuple(("ERPL_IIP_CH_" + c, getattr(_abi, "IIP_CH_" + c)) for c in CHANNELS)
    H.check_struct_layouts(tmp_path, (("erpl_iip_spec", "ErplIipSpec"),), macros)
    assert [getattr(_abi, "IIP_" + r) for r in ROWS] == list(range(16))
    assert [getattr(_abi, "IIP_CH_" + c) for c in CHANNELS] == list(range(5))
    assert _abi.IIP_DIM == _abi.SUMMARY_DIM == 16 and _abi.IIP_MAX_NODES == _abi.CORRIDOR_MAX_NODES and _abi.ABI_VERSION == 4
    assert _abi.IIP_CH_COUNT <= _abi.CORRIDOR_MAX_CHANNELS      # erpl_mc_corridor_bands takes the matrix as it is


def test_defaults(lib):
    s = _abi.ErplIipSpec()
    C.memset(C.byref(s), 0xFF, C.sizeof(s))
    assert lib.erpl_mc_impact_points_defaults(C.byref(s)) == 0
    assert (s.n_nodes, s.record_stride, s.max_steps, s.n_vertices) == (64, 1, 20000, 0)
    assert (s.dt, s.ground, s.drag_scale, s.origin_x, s.origin_y) == (0.05, 0.0, 1.0, 0.0, 0.0)
    assert not any(s.keep_x) and not any(s.keep_y)
    assert lib.erpl_mc_impact_points_defaults(None) == -1 and "spec" in lib.erpl_mc_last_error().decode()


def good(lib):
    """A batch, an out and a spec that pass every check: only the context is left."""
    b, o, s = _abi.ErplBatch(), _abi.ErplOut(), _abi.ErplIipSpec()
    b.n, b.precision, b.k_wind = 8, _abi.PREC_F64_FAST, 6
    b.rocket = b.motor = b.alt_grid = b.wind = DUMMY
    o.n_traj, o.traj_cap = 3, 100
    o.traj_ids = o.traj = o.traj_len = DUMMY
    assert lib.erpl_mc_impact_points_defaults(C.byref(s)) == 0
    s.n_vertices = 3
    s.keep_x[:3], s.keep_y[:3] = [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
    return b, o, s


def test_argument_checks_come_before_any_device_work_in_the_stated_order(lib):
    def call(b, o, s, values=H.DUMMY, ld=10, col0=2):
        ref = lambda x: C.byref(x) if x is not None else None
        rc = lib.erpl_mc_impact_points(None, ref(b), ref(o), ref(s), values, ld, col0, None, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(word, batch=(), out=(), spec=(), rc_want=-1, **kw):
        """`word` names the refused argument although everything that is checked LATER is wrong too."""
        b, o, s = good(lib)
        for obj, sets in ((b, batch), (o, out), (s, spec)):
            for k, v in sets:
                if isinstance(k, tuple):
                    getattr(obj, k[0])[k[1]] = v
                else:
                    setattr(obj, k, v)
        rc, msg = call(b, o, s, **kw)
        assert rc == rc_want and word in msg, (word, msg)

    nan, inf = float("nan"), float("inf")
    # everything behind the argument under test is broken as well: the message shows which check came first
    later_out = [("traj_cap", 0), ("traj_ids", None), ("traj", None), ("traj_len", None)]
    later_batch = [("rocket", None), ("motor", None), ("k_wind", 2000)]
    spec_fields = [("n_nodes", 0), ("record_stride", 0), ("max_steps", 0), ("n_vertices", 2), ("dt", 0.0), ("ground", nan),
                   ("drag_scale", -1.0), ("origin_x", inf), ("origin_y", nan), (("keep_x", 0), nan)]
    behind_spec = dict(batch=[("precision", _abi.PREC_F32), ("n", 0)] + later_batch, out=[("n_traj", -1)] + later_out, col0=-1, ld=0)
    # 1. the four pointers
    b, o, s = good(lib)
    for args, word in (((None, None, None, None), "batch"), ((b, None, None, None), "out"), ((b, o, None, None), "spec"),
                       ((b, o, s, None), "values")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (word, msg)
    refused("values", spec=spec_fields, values=None, **behind_spec)
    # 2. the spec fields in struct order, each against its range
    bad_values = {"n_nodes": (0, -3, _abi.IIP_MAX_NODES + 1), "record_stride": (0, -1), "max_steps": (0, _abi.IIP_MAX_STEPS + 1),
                  "n_vertices": (1, 2, -1, _abi.IIP_MAX_VERTICES + 1), "dt": (0.0, -0.05, nan, inf), "ground": (nan, inf, -inf),
                  "drag_scale": (-1e-9, nan, inf), "origin_x": (nan, -inf), "origin_y": (inf, nan)}
    for i, (name, _) in enumerate(spec_fields[:9]):
        for bad in bad_values[name]:
            refused(name, spec=[(name, bad)] + spec_fields[i + 1:], **behind_spec)
    # 3. a keep-in vertex that is not finite (only the first n_vertices are looked at)
    for arr, bad in (("keep_x", nan), ("keep_y", inf), ("keep_y", -inf)):
        refused("vertex 2", spec=[((arr, 2), bad)], **behind_spec)
    refused("ctx", spec=[(("keep_x", 3), nan), (("keep_y", 63), inf)])
    refused("ctx", spec=[("n_vertices", 0), (("keep_x", 0), nan)])
    # 4. the precision, then the batch size
    rest = dict(out=[("n_traj", -1)] + later_out, col0=-1, ld=0)
    for bad in (_abi.PREC_F32, 3, -1):
        refused("precision", batch=[("precision", bad), ("n", 0)] + later_batch, **rest)
    for bad in (0, -5):
        refused(f"n = {bad}", batch=[("n", bad)] + later_batch, **rest)
    # 5. n_traj, col0, ld
    for bad in (-1, 1 << 31, 1 << 40):
        refused(f"n_traj = {bad}", batch=later_batch, out=[("n_traj", bad)] + later_out, col0=-1, ld=0)
    refused("col0 = -1", batch=later_batch, out=later_out, col0=-1, ld=0)
    refused("ld = 4", batch=later_batch, out=later_out, col0=2, ld=4)         # 2 + 3 columns do not fit 4
    refused("ld = 0", batch=later_batch, out=[("n_traj", 0)] + later_out, col0=1, ld=0)   # checked without trajectories too
    big = (1 << 63) - 1
    refused(f"ld = {big}", batch=later_batch, out=later_out, col0=big - 1, ld=big)        # col0 + n_traj would overflow
    refused("ld = -1", batch=later_batch, out=[("n_traj", 0)] + later_out, col0=0, ld=-1)
    # 6. with trajectories: the capture, then the batch's tables (the envelope's order)
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
    # 7. only the context is left: both fp64 precisions, the extremes of every range, no wind table, exact fit of the columns
    for prec in (_abi.PREC_F64, _abi.PREC_F64_FAST):
        refused("ctx", batch=[("precision", prec)])
    refused("ctx", spec=[("n_nodes", _abi.IIP_MAX_NODES), ("record_stride", (1 << 31) - 1), ("max_steps", _abi.IIP_MAX_STEPS),
                         ("n_vertices", 0), ("dt", 5e-324), ("ground", -1e300), ("drag_scale", 0.0)], ld=5, col0=2)
    refused("ctx", spec=[("n_nodes", 1), ("max_steps", 1), ("n_vertices", _abi.IIP_MAX_VERTICES)],
            batch=[("k_wind", 0), ("alt_grid", None), ("wind", None)], out=[("n_traj", (1 << 31) - 1)], ld=1 << 31, col0=1)
    # without trajectories nothing of the capture or the tables is looked at; the context still is
    refused("ctx", batch=later_batch, out=[("n_traj", 0)] + later_out)


def test_engine_method_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.impact_points: the refusal is on the host, before the library is called (the
    engine here has no library and no context, and there is no batch)."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    ids, tlen = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="traj"):
        TrajectoryEngine.impact_points(eng, None, ids, torch.zeros((2, 4, 15), dtype=torch.float64), tlen)
    with pytest.raises(ValueError, match="traj"):
        TrajectoryEngine.impact_points(eng, None, ids, None, tlen)


def test_python_layer_checks_its_integers_before_a_32_bit_field_can_truncate_them():
    """Device tensors cannot be made here; the refusals that need none are those of MonteCarloAnalyzer.impact_point_trace,
    which come before any engine exists: a stride of 0 is a ValueError as in the sibling methods, not a division by zero."""
    from erpl_monte_carlo_sim_amd import models
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    for kw in (dict(stride=0), dict(nodes=0), dict(nodes=2 ** 32 + 5), dict(record_stride=0)):
        with pytest.raises(ValueError):
            mc.impact_point_trace({}, 8, **kw)
    with pytest.raises(ValueError):
        mc.impact_point_trace({}, 0)


def test_names():
    assert len(analysis.IIP_NAMES) == _abi.IIP_DIM == 16 and len(set(analysis.IIP_NAMES)) == 16
    assert len(analysis.IIP_CHANNELS) == _abi.IIP_CH_COUNT == 5 and len(set(analysis.IIP_CHANNELS)) == 5
    assert all(isinstance(s, str) and s for s in analysis.IIP_NAMES + analysis.IIP_CHANNELS)
    assert analysis.IIP_NAMES[_abi.IIP_MAX_RANGE] == "max_range" and analysis.IIP_NAMES[_abi.IIP_EXIT_TIME] == "exit_time"
    assert analysis.IIP_NAMES[_abi.IIP_NODES] == "nodes" and analysis.IIP_CHANNELS[_abi.IIP_CH_TFALL] == "fall_time"
