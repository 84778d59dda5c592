"""erpl_mc_corridor_defaults / _resample / _bands at the C boundary, as far as it goes without a GPU: the declarations, the
spec and the constants against gcc, the defaults, every argument check in the order the header states (they come before
any device work and look at the context last, so a NULL context and dummy pointers that are never dereferenced show them
all), the host-side refusals of the engine methods and the channel names of the analysis layer."""
import ctypes as C
import os

import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = H.DUMMY.value
NAMES = ("erpl_mc_corridor_defaults", "erpl_mc_corridor_resample", "erpl_mc_corridor_bands")
CHANNELS = ("X", "Y", "Z", "DOWNRANGE", "VX", "VY", "VZ", "SPEED")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_symbols_are_declared_listed_documented_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def test_spec_and_constants_match_the_c_compiler(tmp_path):
    macros = (("ERPL_CORRIDOR_MAX_CHANNELS", _abi.CORRIDOR_MAX_CHANNELS), ("ERPL_CORRIDOR_MAX_NODES", _abi.CORRIDOR_MAX_NODES),
              ("ERPL_CORRIDOR_HOLD_END", _abi.CORRIDOR_HOLD_END), ("ERPL_CH_COUNT", _abi.CH_COUNT)) + \
        tuple(("ERPL_CH_" + c, getattr(_abi, "CH_" + c)) for c in CHANNELS)
    H.check_struct_layouts(tmp_path, (("erpl_corridor_spec", "ErplCorridorSpec"), ("erpl_row_stats", "ErplRowStats")), macros)
    assert [getattr(_abi, "CH_" + c) for c in CHANNELS] == list(range(8)) and _abi.CH_COUNT == 8
    assert _abi.CORRIDOR_MAX_CHANNELS == 8 and _abi.CORRIDOR_MAX_NODES == 4096 and _abi.CORRIDOR_HOLD_END == 1
    assert _abi.ABI_VERSION == 4
    # the engine reads an array of erpl_row_stats as 29 eight-byte words per record
    assert C.sizeof(_abi.ErplRowStats) == 8 * (5 + 3 * _abi.ANALYSIS_MAX_Q)


def test_defaults(lib):
    s = _abi.ErplCorridorSpec()
    C.memset(C.byref(s), 0xff, C.sizeof(s))
    assert lib.erpl_mc_corridor_defaults(C.byref(s)) == 0
    assert s.n_channels == 3 and list(s.channels) == [_abi.CH_Z, _abi.CH_DOWNRANGE, _abi.CH_SPEED, 0, 0, 0, 0, 0]
    assert s.n_nodes == 256 and s.flags == 0 and s.t0 == 0.0 and s.dt == 1.0 and s.reserved == 0
    assert s.n_q == 5 and list(s.q) == [0.05, 0.25, 0.5, 0.75, 0.95, 0.0, 0.0, 0.0]
    assert lib.erpl_mc_corridor_defaults(None) == -1 and "spec" in lib.erpl_mc_last_error().decode()


def good(lib):
    """A spec and an out that pass every check: only the context is left."""
    s, o = _abi.ErplCorridorSpec(), _abi.ErplOut()
    assert lib.erpl_mc_corridor_defaults(C.byref(s)) == 0
    o.n_traj, o.traj_cap = 3, 100
    o.traj = o.traj_len = DUMMY
    return s, o


# spec fields in the order they are checked: (what the message names, how to break the field)
def _set(name, value):
    return lambda s: setattr(s, name, value)


def _set_at(name, j, value):
    return lambda s: getattr(s, name).__setitem__(j, value)


def _twice(s):
    s.channels[2] = s.channels[0]


SPEC_BREAKS = (
    ("n_channels", _set("n_channels", 0)), ("n_channels", _set("n_channels", 9)),
    ("channels[1]", _set_at("channels", 1, 8)), ("channels[0]", _set_at("channels", 0, -1)),
    ("listed twice", _twice),
    ("n_nodes", _set("n_nodes", 0)), ("n_nodes", _set("n_nodes", 4097)),
    ("flags", _set("flags", 2)),
    ("t0", _set("t0", float("nan"))), ("t0", _set("t0", float("inf"))),
    ("dt", _set("dt", 0.0)), ("dt", _set("dt", -1.0)), ("dt", _set("dt", float("nan"))), ("dt", _set("dt", float("inf"))),
    ("n_q", _set("n_q", -1)), ("n_q", _set("n_q", 9)),
    ("q[1]", _set_at("q", 1, 1.5)), ("q[0]", _set_at("q", 0, float("nan"))),
)
# the position of every break in the order of the checks (breaks of one field share a position)
SPEC_ORDER = ("n_channels", "channels", "listed twice", "n_nodes", "flags", "t0", "dt", "n_q", "q[")


def _position(word):
    return next(k for k, w in enumerate(SPEC_ORDER) if word.startswith(w))


def _spec_cases(lib):
    """Every spec break together with ONE break of every field that is checked later."""
    for word, brk in SPEC_BREAKS:
        s, _ = good(lib)
        seen = set()
        for later_word, later in reversed(SPEC_BREAKS):
            p = _position(later_word)
            if p > _position(word) and p not in seen and later_word != "listed twice":
                later(s)
                seen.add(p)
        brk(s)
        yield word, s


def test_resample_checks_come_before_any_device_work_in_the_stated_order(lib):
    def call(s, o, values=H.DUMMY, ld=10, col0=2):
        rc = lib.erpl_mc_corridor_resample(None, C.byref(o) if o is not None else None, C.byref(s) if s is not None else None,
                                           values, ld, col0, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(word, s=None, out=(), **kw):
        """`word` names the refused argument although everything that is checked LATER is wrong too."""
        gs, o = good(lib)
        for k, v in out:
            setattr(o, k, v)
        rc, msg = call(s if s is not None else gs, o, **kw)
        assert rc == -1 and word in msg, (word, msg)

    later_out = [("traj_cap", 0), ("traj", None), ("traj_len", None)]
    # 1. the spec, before everything else
    rc, msg = call(None, None, None, -1, -1)
    assert rc == -1 and "spec" in msg
    for word, s in _spec_cases(lib):
        rc, msg = call(s, None, None, -1, -1)
        assert rc == -1 and word in msg and "spec->" in msg, (word, msg)
    # 2. out
    rc, msg = call(good(lib)[0], None, None, -1, -1)
    assert rc == -1 and "out" in msg
    # 3. n_traj, col0, ld
    for bad in (-1, 1 << 31, 1 << 40):
        refused(f"n_traj = {bad}", out=[("n_traj", bad)] + later_out, values=None, ld=-1, col0=-1)
    refused("col0 = -1", out=later_out, values=None, ld=-1, col0=-1)
    refused("ld = 4", out=later_out, values=None, ld=4, col0=2)          # 2 + 3 > 4
    refused("ld = 2", out=later_out, values=None, ld=2, col0=0)          # below n_traj itself
    refused("ld = 9", out=[("n_traj", (1 << 31) - 1)] + later_out, values=None, ld=9, col0=(1 << 62))   # no overflow
    # 4. values
    refused("values", out=later_out, values=None, ld=5, col0=2)
    # 5. with trajectories: the capture
    refused("traj_cap", out=later_out)
    refused("traj is NULL", out=later_out[1:])
    refused("traj_len", out=later_out[2:])
    # 6. only the context is left
    refused("ctx")
    refused("ctx", ld=5, col0=2)
    s, _ = good(lib)
    s.flags, s.n_q, s.n_nodes, s.n_channels = _abi.CORRIDOR_HOLD_END, 0, 4096, 8
    s.channels[:] = [7, 6, 5, 4, 3, 2, 1, 0]
    refused("ctx", s=s)
    # without trajectories nothing of the capture is looked at; the context still is
    refused("ctx", out=[("n_traj", 0)] + later_out, ld=0, col0=0)


def test_bands_checks_come_before_any_device_work_in_the_stated_order(lib):
    def call(s, values=H.DUMMY, bands=H.DUMMY, m=5, ld=5):
        rc = lib.erpl_mc_corridor_bands(None, values, None, m, ld, C.byref(s) if s is not None else None, bands, None, None)
        return rc, lib.erpl_mc_last_error().decode()

    gs = good(lib)[0]
    rc, msg = call(None, None, None, 0, -1)
    assert rc == -1 and "spec" in msg
    for word, s in _spec_cases(lib):
        rc, msg = call(s, None, None, 0, -1)
        assert rc == -1 and word in msg and "spec->" in msg, (word, msg)
    for bad in (0, -3, 1 << 31):
        rc, msg = call(gs, None, None, bad, -1)
        assert rc == -1 and f"m = {bad}" in msg, msg
    rc, msg = call(gs, None, None, 5, 4)
    assert rc == -1 and "ld = 4" in msg, msg
    rc, msg = call(gs, None, None)
    assert rc == -1 and "values" in msg, msg
    rc, msg = call(gs, H.DUMMY, None)
    assert rc == -1 and "bands" in msg, msg
    for m, ld in ((5, 5), (1, 1), ((1 << 31) - 1, 1 << 40)):
        rc, msg = call(gs, m=m, ld=ld)
        assert rc == -1 and "ctx" in msg, msg


def test_engine_methods_refuse_host_tensors():
    """No CPU path behind the corridor calls: the refusals are on the host, before the library is called (the engine here
    has no library and no context)."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    tlen = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="traj"):
        TrajectoryEngine.corridor_resample(eng, torch.zeros((2, 4, 15), dtype=torch.float64), tlen, None, 8, 0.0, 1.0)
    with pytest.raises(ValueError, match="traj"):
        TrajectoryEngine.corridor_resample(eng, None, tlen)
    with pytest.raises(ValueError, match="values"):
        TrajectoryEngine.corridor_bands(eng, torch.zeros((2, 3, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="values"):
        TrajectoryEngine.corridor_bands(eng, None)


def test_channel_names():
    names = analysis.CORRIDOR_CHANNEL_NAMES
    assert len(names) == _abi.CH_COUNT == 8 and len(set(names)) == 8
    assert names == ("x", "y", "z", "downrange", "vx", "vy", "vz", "speed")
    assert names[_abi.CH_Z] == "z" and names[_abi.CH_DOWNRANGE] == "downrange" and names[_abi.CH_SPEED] == "speed"
    assert analysis.corridor_channels(("z", "downrange", _abi.CH_SPEED)) == [2, 3, 7]
    with pytest.raises(ValueError, match="altitude"):
        analysis.corridor_channels(("altitude",))
