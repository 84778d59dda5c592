"""erpl_mc_debris at the C boundary, as far as it goes without a GPU: the declarations, the constants and the layout of
erpl_debris_spec against gcc, the defaults, every argument check in the order the header states (they come before any device
work and look at the context last, so a NULL context and dummy pointers that are never dereferenced show them all), the
host-side refusal of the engine method, the names of the analysis layer and the host check of csrc/erpl_debris.h."""
import ctypes as C
import os
import subprocess

import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
DUMMY = H.DUMMY.value

ROWS = ("MAX_RANGE", "MAX_RANGE_TIME", "MAX_RANGE_X", "MAX_RANGE_Y", "MAX_RANGE_FRAGMENT", "EXIT_TIME", "EXIT_FRAGMENT", "EXIT_X",
        "EXIT_Y", "MAX_TFALL", "MAX_TFALL_TIME", "MAX_SPREAD", "MAX_SPREAD_TIME", "OUTSIDE", "LANDED", "NODES")
NAMES = ("erpl_mc_debris_defaults", "erpl_mc_debris", "erpl_mc_debris_directions_host")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_symbols_are_declared_listed_documented_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc
        getattr(lib, name)
    philox = open(os.path.join(CSRC, "erpl_philox.h")).read()
    assert "5 the break-up directions of erpl_mc_debris" in philox      # the list of family tags knows the new one


def test_constants_and_struct_layout_match_the_c_compiler(tmp_path):
    macros = (("ERPL_DEBRIS_DIM", _abi.DEBRIS_DIM), ("ERPL_DEBRIS_MAX_FRAGMENTS", _abi.DEBRIS_MAX_FRAGMENTS),
              ("ERPL_DEBRIS_MAX_HALVINGS", _abi.DEBRIS_MAX_HALVINGS))
    macros += tuple(("ERPL_DEBRIS_" + r, getattr(_abi, "DEBRIS_" + r)) for r in ROWS)
    H.check_struct_layouts(tmp_path, (("erpl_debris_spec", "ErplDebrisSpec"),), macros)
    assert [getattr(_abi, "DEBRIS_" + r) for r in ROWS] == list(range(16))
    assert _abi.DEBRIS_DIM == _abi.SUMMARY_DIM == 16 and _abi.ABI_VERSION == 4
    assert _abi.DEBRIS_MAX_FRAGMENTS == 64 and _abi.DEBRIS_MAX_HALVINGS == 16
    assert _abi.IIP_CH_COUNT <= _abi.CORRIDOR_MAX_CHANNELS      # erpl_mc_corridor_bands takes the matrix as it is


def test_defaults(lib):
    s = _abi.ErplDebrisSpec()
    C.memset(C.byref(s), 0xFF, C.sizeof(s))
    assert lib.erpl_mc_debris_defaults(C.byref(s)) == 0
    assert (s.n_nodes, s.record_stride, s.max_steps, s.n_vertices, s.n_fragments, s.seed) == (16, 1, 20000, 0, 1, 0)
    assert (s.dt, s.ground, s.origin_x, s.origin_y, s.stiff_limit) == (0.05, 0.0, 0.0, 0.0, 0.25)
    assert s.beta[0] == float("inf") and not any(s.beta[1:]) and not any(s.dv) and not any(s.keep_x) and not any(s.keep_y)
    assert lib.erpl_mc_debris_defaults(None) == -1 and "spec" in lib.erpl_mc_last_error().decode()


def good(lib):
    """A batch, an out and a spec that pass every check: only the context is left."""
    b, o, s = _abi.ErplBatch(), _abi.ErplOut(), _abi.ErplDebrisSpec()
    b.n, b.precision, b.k_wind = 8, _abi.PREC_F64_FAST, 6
    b.rocket = b.motor = b.alt_grid = b.wind = DUMMY
    o.n_traj, o.traj_cap = 3, 100
    o.traj_ids = o.traj = o.traj_len = DUMMY
    assert lib.erpl_mc_debris_defaults(C.byref(s)) == 0
    s.n_vertices = 3
    s.keep_x[:3], s.keep_y[:3] = [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
    s.n_fragments = 3
    s.beta[:3], s.dv[:3] = [5.0, float("inf"), 200.0], [0.0, 10.0, 30.0]
    return b, o, s


def test_argument_checks_come_before_any_device_work_in_the_stated_order(lib):
    def call(b, o, s, values=H.DUMMY, ld=10, col0=2):
        ref = lambda x: C.byref(x) if x is not None else None
        rc = lib.erpl_mc_debris(None, ref(b), ref(o), ref(s), values, ld, col0, None, None)
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
    later_out = [("traj_cap", 0), ("traj_ids", None), ("traj", None), ("traj_len", None)]
    later_batch = [("rocket", None), ("motor", None), ("k_wind", 2000)]
    # the order of the checks (n_nodes = 4096 with two fragments: each in range, the product is not)
    spec_fields = [("n_nodes", 0), ("record_stride", 0), ("max_steps", 0), ("n_vertices", 2), ("n_fragments", 0), ("dt", 0.0),
                   ("ground", nan), ("origin_x", inf), ("origin_y", nan), ("stiff_limit", 0.0), (("beta", 0), 0.0), (("dv", 0), -1.0),
                   (("keep_x", 0), nan)]
    behind_spec = dict(batch=[("precision", _abi.PREC_F32), ("n", 0)] + later_batch, out=[("n_traj", -1)] + later_out, col0=-1, ld=0)
    # 1. the four pointers
    b, o, s = good(lib)
    for args, word in (((None, None, None, None), "batch"), ((b, None, None, None), "out"), ((b, o, None, None), "spec"),
                       ((b, o, s, None), "values")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (word, msg)
    refused("values", spec=spec_fields, values=None, **behind_spec)
    # 2. the scalar fields in the stated order, each against its range
    bad_values = {"n_nodes": (0, -3, _abi.IIP_MAX_NODES + 1), "record_stride": (0, -1), "max_steps": (0, _abi.IIP_MAX_STEPS + 1),
                  "n_vertices": (1, 2, -1, _abi.IIP_MAX_VERTICES + 1), "n_fragments": (0, -1, _abi.DEBRIS_MAX_FRAGMENTS + 1),
                  "dt": (0.0, -0.05, nan, inf), "ground": (nan, inf, -inf), "origin_x": (nan, -inf), "origin_y": (inf, nan),
                  "stiff_limit": (0.0, -0.25, nan, inf, 1.0000000000000002)}
    for i, (name, _) in enumerate(spec_fields[:10]):
        for bad in bad_values[name]:
            refused(name, spec=[(name, bad)] + spec_fields[i + 1:], **behind_spec)
    # 3. the product of nodes and fragments, behind both of its factors and ahead of dt
    for nodes, frags in ((4096, 2), (65, 64), (2049, 2)):
        refused("n_nodes * n_fragments", spec=[("n_nodes", nodes), ("n_fragments", frags)] + spec_fields[5:], **behind_spec)
    # 4. the fragments in turn: beta then dv of fragment 0, then of fragment 1, ...; only the first n_fragments are looked at
    for bad in (0.0, -2.0, nan, -inf):
        refused("beta of fragment 0", spec=[(("beta", 0), bad)] + spec_fields[11:], **behind_spec)
        refused("beta of fragment 2", spec=[(("beta", 2), bad), (("keep_x", 0), nan)], **behind_spec)
    for bad in (-1e-9, nan, inf, -inf):
        refused("dv of fragment 0", spec=[(("dv", 0), bad), (("beta", 1), 0.0)] + spec_fields[12:], **behind_spec)
        refused("dv of fragment 1", spec=[(("dv", 1), bad), (("beta", 2), 0.0), (("keep_x", 0), nan)], **behind_spec)
    refused("beta of fragment 1", spec=[(("beta", 1), nan), (("dv", 0), 0.0), (("dv", 1), -1.0)], **behind_spec)
    refused("ctx", spec=[(("beta", 3), nan), (("dv", 63), -1.0)])
    # 5. a keep-in vertex that is not finite (only the first n_vertices are looked at)
    for arr, bad in (("keep_x", nan), ("keep_y", inf), ("keep_y", -inf)):
        refused("vertex 2", spec=[((arr, 2), bad)], **behind_spec)
    refused("ctx", spec=[(("keep_x", 3), nan), (("keep_y", 63), inf)])
    refused("ctx", spec=[("n_vertices", 0), (("keep_x", 0), nan)])
    # 6. the precision, then the batch size
    rest = dict(out=[("n_traj", -1)] + later_out, col0=-1, ld=0)
    for bad in (_abi.PREC_F32, 3, -1):
        refused("precision", batch=[("precision", bad), ("n", 0)] + later_batch, **rest)
    for bad in (0, -5):
        refused(f"n = {bad}", batch=[("n", bad)] + later_batch, **rest)
    # 7. n_traj, col0, ld
    for bad in (-1, 1 << 31, 1 << 40):
        refused(f"n_traj = {bad}", batch=later_batch, out=[("n_traj", bad)] + later_out, col0=-1, ld=0)
    refused("col0 = -1", batch=later_batch, out=later_out, col0=-1, ld=0)
    refused("ld = 4", batch=later_batch, out=later_out, col0=2, ld=4)         # 2 + 3 columns do not fit 4
    refused("ld = 0", batch=later_batch, out=[("n_traj", 0)] + later_out, col0=1, ld=0)
    big = (1 << 63) - 1
    refused(f"ld = {big}", batch=later_batch, out=later_out, col0=big - 1, ld=big)
    refused("ld = -1", batch=later_batch, out=[("n_traj", 0)] + later_out, col0=0, ld=-1)
    # 8. with trajectories: the capture, then the batch's tables
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
    # 9. only the context is left: both fp64 precisions, the extremes of every range, no wind table, exact fit of the columns
    for prec in (_abi.PREC_F64, _abi.PREC_F64_FAST):
        refused("ctx", batch=[("precision", prec)])
    refused("ctx", spec=[("n_nodes", 64), ("n_fragments", 64), ("record_stride", (1 << 31) - 1), ("max_steps", _abi.IIP_MAX_STEPS),
                         ("n_vertices", 0), ("dt", 5e-324), ("ground", -1e300), ("stiff_limit", 1.0), ("seed", (1 << 64) - 1)]
            + [(("beta", f), 1e-300) for f in range(64)] + [(("dv", f), 1e300) for f in range(64)], ld=5, col0=2)
    refused("ctx", spec=[("n_nodes", _abi.IIP_MAX_NODES), ("n_fragments", 1), ("max_steps", 1), ("n_vertices", _abi.IIP_MAX_VERTICES),
                         ("stiff_limit", 5e-324), (("beta", 0), inf)],
            batch=[("k_wind", 0), ("alt_grid", None), ("wind", None)], out=[("n_traj", (1 << 31) - 1)], ld=1 << 31, col0=1)
    refused("ctx", batch=later_batch, out=[("n_traj", 0)] + later_out)


def test_directions_host_refusals(lib):
    import numpy as np
    ids, out = np.arange(4, dtype=np.int64), np.zeros((3, 4))
    call = lambda i, n, node, frag, o: lib.erpl_mc_debris_directions_host(1, i, n, node, frag, o)
    assert call(ids.ctypes.data, 4, 0, 0, out.ctypes.data) == 0 and np.isfinite(out).all() and out.any()
    assert call(None, 0, 0, 0, None) == 0
    for args, word in (((ids.ctypes.data, -1, 0, 0, out.ctypes.data), "n = -1"), ((ids.ctypes.data, 4, -1, 0, out.ctypes.data), "node"),
                       ((ids.ctypes.data, 4, 4096, 0, out.ctypes.data), "node"), ((ids.ctypes.data, 4, 0, 64, out.ctypes.data), "fragment"),
                       ((None, 4, 0, 0, out.ctypes.data), "sample_ids"), ((ids.ctypes.data, 4, 0, 0, None), "dir")):
        assert call(*args) == -1 and word in lib.erpl_mc_last_error().decode(), word
    ids[2] = -7
    assert call(ids.ctypes.data, 4, 0, 0, out.ctypes.data) == -1 and "sample_ids[2]" in lib.erpl_mc_last_error().decode()


def test_engine_method_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.debris: the refusal is on the host, before the library is called (the engine here
    has no library and no context, and there is no batch)."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    ids, tlen = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="traj"):
        TrajectoryEngine.debris(eng, None, ids, torch.zeros((2, 4, 15), dtype=torch.float64), tlen, [(5.0, 0.0)])
    with pytest.raises(ValueError, match="traj"):
        TrajectoryEngine.debris(eng, None, ids, None, tlen, [(5.0, 0.0)])


def test_python_layer_checks_its_arguments_before_any_engine_exists():
    from erpl_monte_carlo_sim_amd import models
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    frag = [(5.0, 0.0)]
    for kw in (dict(stride=0), dict(nodes=0), dict(nodes=2 ** 32 + 5), dict(record_stride=0), dict(fragments=[]),
               dict(fragments=[(1.0, 0.0)] * 65), dict(nodes=65, fragments=[(1.0, 0.0)] * 64), dict(fragments=[(0.0, 1.0)]),
               dict(fragments=[(5.0, -1.0)]), dict(maps=[(16, 0)]), dict(maps=[(0, 1)])):
        with pytest.raises(ValueError):
            mc.debris_footprint({}, 8, **{"fragments": frag, **kw})
    with pytest.raises(ValueError):
        mc.debris_footprint({}, 0, fragments=frag)


def test_names():
    assert len(analysis.DEBRIS_NAMES) == _abi.DEBRIS_DIM == 16 and len(set(analysis.DEBRIS_NAMES)) == 16
    assert analysis.DEBRIS_CHANNELS == analysis.IIP_CHANNELS and len(analysis.DEBRIS_CHANNELS) == _abi.IIP_CH_COUNT
    assert all(isinstance(s, str) and s for s in analysis.DEBRIS_NAMES)
    assert analysis.DEBRIS_NAMES[_abi.DEBRIS_MAX_RANGE] == "max_range" and analysis.DEBRIS_NAMES[_abi.DEBRIS_EXIT_TIME] == "exit_time"
    assert analysis.DEBRIS_NAMES[_abi.DEBRIS_MAX_TFALL] == "max_fall_time" and analysis.DEBRIS_NAMES[_abi.DEBRIS_NODES] == "nodes"


def test_the_host_check_program_passes(lib):
    exe = os.path.join(CSRC, "erpl_debris_check")
    assert os.path.exists(exe), "erpl_debris_check is built by `make all` (build())"
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("ok erpl_debris_check") and "FAIL" not in res.stdout
