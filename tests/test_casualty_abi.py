"""erpl_mc_casualty at the C boundary, as far as it goes without a GPU: the declarations, the constants and the layout of its
two structs against gcc, the defaults, every argument check in the order the header states (they come before any device work
and look at the context last, so a NULL context and dummy pointers that are never dereferenced show them all), the refusals of
the Python layers and the host check of csrc/erpl_casualty.h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
NAMES = ("erpl_mc_casualty_defaults", "erpl_mc_casualty")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_symbols_are_declared_listed_documented_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc
        getattr(lib, name)
    assert "cannot hide a hazard" in hdr       # the header says why a missing job counts as zero and is reported


def test_constants_and_struct_layout_match_the_c_compiler(tmp_path):
    macros = (("ERPL_CASUALTY_MAX_GRID", _abi.CASUALTY_MAX_GRID), ("ERPL_CASUALTY_MAX_LEVELS", _abi.CASUALTY_MAX_LEVELS),
              ("ERPL_CASUALTY_SPLIT_DIM", _abi.CASUALTY_SPLIT_DIM), ("ERPL_CASUALTY_GROUP_DIM", _abi.CASUALTY_GROUP_DIM))
    macros += tuple(("ERPL_CASUALTY_" + r, getattr(_abi, "CASUALTY_" + r)) for r in
                    ("EC", "LANDED", "LETHAL", "OFF_GRID", "MISSING", "G_COUNT", "G_S", "G_MEAN_X", "G_MEAN_Y", "G_HXX", "G_HXY",
                     "G_HYY", "G_W"))
    H.check_struct_layouts(tmp_path, (("erpl_casualty_spec", "ErplCasualtySpec"), ("erpl_casualty", "ErplCasualty")), macros)
    assert _abi.CASUALTY_MAX_GRID == 1024 and _abi.CASUALTY_MAX_LEVELS == 8 and _abi.ABI_VERSION == 4
    assert len(analysis.CASUALTY_COUNTS) + 1 == _abi.CASUALTY_SPLIT_DIM


def test_defaults(lib):
    s = _abi.ErplCasualtySpec()
    C.memset(C.byref(s), 0xFF, C.sizeof(s))
    assert lib.erpl_mc_casualty_defaults(C.byref(s)) == 0
    assert (s.n_nodes, s.n_fragments, s.bins_x, s.bins_y, s.smooth, s.n_levels) == (16, 1, 64, 64, 1, 2)
    assert (s.ke_min, s.lo_x, s.hi_x, s.lo_y, s.hi_y, s.bw_scale, s.h_floor) == (15.0, -1000.0, 1000.0, -1000.0, 1000.0, 1.0, 1.0)
    assert list(s.level[:2]) == [1e-6, 1e-5] and not any(s.level[2:])
    assert (s.pieces[0], s.area[0], s.mass[0]) == (1.0, 1.0, 1.0) and not any(s.pieces[1:]) and not any(s.area[1:]) and not any(s.mass[1:])
    assert lib.erpl_mc_casualty_defaults(None) == -1 and "spec" in lib.erpl_mc_last_error().decode()


def good(lib):
    s = _abi.ErplCasualtySpec()
    assert lib.erpl_mc_casualty_defaults(C.byref(s)) == 0
    s.n_nodes, s.n_fragments = 4, 3
    for f in range(3):
        s.pieces[f], s.area[f], s.mass[f] = 2.0 + f, 0.5, 10.0 * f
    return s, (C.c_double * 4)(0.1, 0.2, 0.0, 0.3)


def check_refusals(lib):
    """Every refusal that needs no device work, in the order of the header.  The context is NULL: the pointers that stand in
    for device memory are never dereferenced, and a call that passes every other check ends at the context."""
    def call(s, p, values=H.DUMMY, population=H.DUMMY, result=True, ld=10, m=8):
        res = _abi.ErplCasualty()
        rc = lib.erpl_mc_casualty(None, values, ld, m, None, C.byref(s) if s is not None else None, p, population, None, None, None,
                                  None, None, None, None, C.byref(res) if result else None, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(word, spec=(), p=None, **kw):
        """`word` names the refused argument although everything that is checked LATER is wrong too."""
        s, pf = good(lib)
        for k, v in spec:
            if isinstance(k, tuple):
                getattr(s, k[0])[k[1]] = v
            else:
                setattr(s, k, v)
        for k, v in (p or ()):
            pf[k] = v
        rc, msg = call(s, pf, **kw)
        assert rc == -1 and word in msg, (word, msg)

    nan, inf = float("nan"), float("inf")
    s, pf = good(lib)
    # 1. the five pointers
    for kw, word in ((dict(values=None, population=None, result=False), "values"), (dict(population=None, result=False), "population"),
                     (dict(result=False), "result")):
        rc, msg = call(s, pf, **kw)
        assert rc == -1 and word in msg, (word, msg)
    for args, word in (((None, None), "spec"), ((s, None), "p_fail")):
        rc, msg = call(*args, population=None, result=False)
        assert rc == -1 and word in msg, (word, msg)
    rc, msg = call(None, None, values=None)
    assert rc == -1 and "values" in msg
    # 2. - 9. the fields of the spec in the stated order, each ahead of everything behind it
    fields = [("n_nodes", 0), ("n_fragments", 0), (("pieces", 0), -1.0), (("area", 0), nan), (("mass", 0), inf), ("ke_min", -1.0),
              ("bins_x", 0), ("bins_y", 1025), ("lo_x", 5000.0), ("lo_y", nan), ("smooth", 2), ("bw_scale", 0.0), ("h_floor", -1.0),
              (("level", 0), 1.0)]
    behind = dict(p=[(0, -0.5)], m=0, ld=-1)
    bad = {"n_nodes": (0, -1, _abi.IIP_MAX_NODES + 1), "n_fragments": (0, -2, _abi.DEBRIS_MAX_FRAGMENTS + 1), "ke_min": (-1e-300, nan, inf),
           "bins_x": (0, -1, 1025), "bins_y": (0, 1025), "lo_x": (1000.0, nan, -inf), "lo_y": (1000.0, inf), "smooth": (-1, 2),
           "bw_scale": (0.0, -1.0, nan, inf), "h_floor": (0.0, nan, inf)}
    for i, (name, _) in enumerate(fields):
        if isinstance(name, tuple):
            continue
        for v in bad[name]:
            refused(name, spec=[(name, v)] + fields[i + 1:], **behind)
    for nodes, frags in ((4096, 2), (65, 64)):
        refused("n_nodes * n_fragments", spec=[("n_nodes", nodes), ("n_fragments", frags)] + fields[2:], **behind)
    # per fragment pieces, then area, then mass; only the first n_fragments are looked at
    for v in (-1.0, nan, inf, -inf):
        refused("pieces[0]", spec=[(("pieces", 0), v)] + fields[3:], **behind)
        refused("area[0]", spec=[(("area", 0), v), (("mass", 0), nan), (("pieces", 1), nan)] + fields[5:], **behind)
        refused("mass[0]", spec=[(("mass", 0), v), (("pieces", 1), nan)] + fields[5:], **behind)
        refused("pieces[2]", spec=[(("pieces", 2), v), (("area", 2), nan)] + fields[5:], **behind)
    refused("ctx", spec=[(("pieces", 3), nan), (("mass", 63), -1.0)])
    refused("hi_x", spec=[("hi_x", inf)] + fields[9:], **behind)
    refused("hi_y", spec=[("hi_y", -2000.0)] + fields[10:], **behind)
    for v in (0.0, 1.0, -0.1, nan):
        refused("level[1]", spec=[(("level", 1), v)], **behind)
    refused("n_levels", spec=[("n_levels", 9), (("level", 0), 2.0)], **behind)
    refused("ctx", spec=[("n_levels", 1), (("level", 1), 7.0)])
    # 10. p_fail
    for v in (-1e-9, nan, inf):
        refused("p_fail[2]", p=[(2, v)], m=0, ld=-1)
    refused("p_fail sums", p=[(2, 0.4 + 1e-9)], m=0, ld=-1)
    refused("ctx", p=[(2, 0.4)])                                       # sums to 1 exactly
    # 11. m, 12. ld
    for v in (0, -1, 1 << 31, 1 << 40):
        refused(f"m = {v}", m=v, ld=-1)
    refused("ld = 7", m=8, ld=7)


def test_argument_checks_come_before_any_device_work_in_the_stated_order(lib):
    check_refusals(lib)
    s, _ = good(lib)
    s.n_nodes, s.n_fragments, s.n_levels, s.smooth, s.ke_min = 64, 64, 0, 0, 0.0
    pf = (C.c_double * 64)(*([0.0] * 64))
    res = _abi.ErplCasualty()
    rc = lib.erpl_mc_casualty(None, H.DUMMY, (1 << 31) - 1, (1 << 31) - 1, None, C.byref(s), pf, H.DUMMY, None, None, None, None, None,
                              None, None, C.byref(res), None)
    assert rc == -1 and "ctx" in lib.erpl_mc_last_error().decode()     # the largest shape: Q = 19, not refused


def test_python_layers_refuse_before_any_engine_exists():
    frag = [(1.0, 1.0, 1.0)]
    rng = ((-1.0, 1.0), (-1.0, 1.0))
    spec = analysis.casualty_spec(4, frag * 3, (8, 6), rng, levels=(1e-6,))
    assert (spec.n_nodes, spec.n_fragments, spec.bins_x, spec.bins_y, spec.n_levels, spec.smooth) == (4, 3, 8, 6, 1, 1)
    for kw in (dict(n_nodes=0), dict(n_nodes=2 ** 32 + 4), dict(fragments=[]), dict(fragments=frag * 65), dict(n_nodes=65, fragments=frag * 64),
               dict(fragments=[(1.0, 1.0)]), dict(fragments=[(-1.0, 1.0, 1.0)]), dict(fragments=[(1.0, float("nan"), 1.0)]),
               dict(bins=(0, 4)), dict(bins=(2 ** 32 + 8, 4)), dict(bins=(4, 1025)), dict(ranges=((1.0, 1.0), (-1.0, 1.0))),
               dict(ranges=((-1.0, 1.0), (0.0, float("inf")))), dict(ke_min=-1.0), dict(bw_scale=0.0), dict(h_floor=float("nan")),
               dict(levels=(0.0,)), dict(levels=(1e-6,) * 9), dict(levels=(1.0,))):
        args = dict(n_nodes=4, fragments=frag, bins=(8, 6), ranges=rng)
        args.update(kw)
        with pytest.raises(ValueError):
            analysis.casualty_spec(**args)

    from erpl_monte_carlo_sim_amd import models
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    foot = {"fragments": [(5.0, 0.0), (50.0, 1.0)], "time": np.arange(4.0), "values": None, "reasons": None}
    pop = np.zeros((8, 6))
    two = [(1.0, 1.0, 1.0), (2.0, 0.5, 3.0)]
    for kw in (dict(fragments=frag, p_fail=[0.1] * 4), dict(fragments=two), dict(fragments=two, p_fail=[0.1] * 4, failure_rate=0.01),
               dict(fragments=two, p_fail=[0.1] * 3), dict(fragments=two, p_fail=[0.1] * 4, levels=(2.0,)),
               dict(fragments=two, failure_rate=-1.0), dict(fragments=two, p_fail=[0.1] * 4, ke_min=float("nan"))):
        with pytest.raises(ValueError):
            mc.casualty_expectation(foot, pop, rng, **kw)
    with pytest.raises(ValueError):
        mc.casualty_expectation(foot, np.zeros(8), rng, fragments=two, p_fail=[0.1] * 4)


def test_engine_method_refuses_host_tensors():
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="values"):
        TrajectoryEngine.casualty(eng, torch.zeros((5, 4, 8), dtype=torch.float64), [(1.0, 1.0, 1.0)], [0.1] * 4, None, None)
    with pytest.raises(ValueError, match="values"):
        TrajectoryEngine.casualty(eng, None, [(1.0, 1.0, 1.0)], [0.1] * 4, None, None)


def test_failure_probabilities():
    t = np.array([0.0, 10.0, 20.0, 30.0])
    p = analysis.failure_probabilities(t, 0.01)
    np.testing.assert_allclose(p, np.exp(-0.01 * t) - np.exp(-0.01 * (t + 10.0)), rtol=1e-15)
    assert abs(p.sum() - (1.0 - np.exp(-0.4))) < 1e-15
    p = analysis.failure_probabilities(t + 5.0, [0.02, 0.0, 0.01, 0.03], t_end=50.0)     # the rate of node 0 also holds before it
    L = np.array([0.1, 0.3, 0.3, 0.4, 0.85])
    np.testing.assert_allclose(p, np.exp(-L[:-1]) - np.exp(-L[1:]), rtol=1e-14, atol=1e-18)
    assert p[1] == 0.0 and p.sum() <= 1.0
    assert analysis.failure_probabilities([3.0], 0.5, t_end=4.0).shape == (1,)
    for args in (([3.0], 0.5), ([0.0, 1.0], -0.1), ([1.0, 1.0], 0.1), ([0.0, 1.0], [0.1]), ([-1.0, 1.0], 0.1), ([0.0, 1.0], 0.1, 1.0)):
        with pytest.raises(ValueError):
            analysis.failure_probabilities(*args)


def test_the_host_check_program_passes(lib):
    exe = os.path.join(CSRC, "erpl_casualty_check")
    assert os.path.exists(exe), "erpl_casualty_check is built by `make all` (build())"
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("ok erpl_casualty_check") and "FAIL" not in res.stdout
