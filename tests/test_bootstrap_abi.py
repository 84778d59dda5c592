"""erpl_mc_bootstrap, its defaults and erpl_mc_bootstrap_indices at the C boundary, as far as it goes without a GPU: the
tests' own Philox against the Random123 known answers, struct layouts against gcc, the defaults, every argument check (they
come before any device work, in the order the header lists, and look at the context last: a NULL context and a dummy
pointer that is never dereferenced show them all) and the host copy of the draws against philox_ref."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

import philox_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = H.DUMMY

STRUCTS = (("erpl_boot_spec", "ErplBootSpec"), ("erpl_boot_stat", "ErplBootStat"), ("erpl_bootstrap", "ErplBootstrap"))
MACROS = (("ERPL_BOOT_MAX_ROWS", _abi.BOOT_MAX_ROWS), ("ERPL_BOOT_ROW_EXTRA", _abi.BOOT_ROW_EXTRA),
          ("ERPL_BOOT_MAX_REPLICATES", _abi.BOOT_MAX_REPLICATES), ("ERPL_BOOT_MAX_STATS", _abi.BOOT_MAX_STATS))


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_philox_ref_reproduces_the_random123_known_answers():
    """The three philox4x32-10 vectors of Random123's kat_vectors."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for counter, key, want in kat:
        got = philox_ref.philox4x32_10(counter, key)
        assert tuple(int(w[0]) for w in got) == want
    # vectorised: the three at once through the counter arrays, one key
    got = philox_ref.philox4x32_10(([0, 5], [0, 6], [0, 7], [0, 8]), (0, 0))
    assert tuple(int(w[0]) for w in got) == kat[0][2]
    assert philox_ref.indices(0, 0, 5).tolist() == [4, 3, 1, 0, 1]
    assert philox_ref.indices(1234, 7, 9).tolist() == [1, 1, 6, 0, 1, 3, 6, 8, 0]


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and the offset of EVERY field of the three ctypes mirrors == what gcc sees in include/erpl_mc.h."""
    H.check_struct_layouts(tmp_path, STRUCTS, MACROS)
    assert (_abi.BOOT_MAX_ROWS, _abi.BOOT_ROW_EXTRA, _abi.BOOT_MAX_REPLICATES, _abi.BOOT_MAX_STATS) == (4, 16, 65536, 40)
    assert _abi.BOOT_ROW_EXTRA == _abi.SUMMARY_DIM and _abi.ABI_VERSION == 4


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_bootstrap_defaults", "erpl_mc_bootstrap", "erpl_mc_bootstrap_indices"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def defaults(lib):
    spec = _abi.ErplBootSpec()
    assert lib.erpl_mc_bootstrap_defaults(C.byref(spec)) == 0
    return spec


def test_defaults_are_exact(lib):
    spec = _abi.ErplBootSpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_bootstrap_defaults(C.byref(spec)) == 0
    assert spec.n_rows == 3 and list(spec.rows) == [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, 0]
    ana = _abi.ErplAnalysisSpec()
    assert lib.erpl_mc_analysis_defaults(C.byref(ana)) == 0
    assert spec.n_q == ana.n_q == 5 and list(spec.q) == list(ana.q) == [0.05, 0.25, 0.5, 0.75, 0.95, 0.0, 0.0, 0.0]
    assert spec.replicates == 2000 and spec.level == 0.95 and spec.seed == 0 and spec.reserved == 0
    assert lib.erpl_mc_bootstrap_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_argument_checks_come_before_any_device_work_in_the_documented_order(lib):
    res = _abi.ErplBootstrap()

    def call(spec, n=8, summary=DUMMY, extra=None, result=res, rep=None):
        rc = lib.erpl_mc_bootstrap(None, summary, extra, None, n, C.byref(spec) if spec is not None else None,
                                   C.byref(result) if result is not None else None, rep, None)
        return rc, lib.erpl_mc_last_error().decode()

    def broken(**fields):
        """A spec with EVERY later check failing too: the earlier one has to be the one reported."""
        spec = defaults(lib)
        spec.level = 1.0
        for k, v in fields.items():
            setattr(spec, k, v)
        return spec

    # NULL spec, summary, result - in this order, whatever else is wrong
    rc, msg = call(None, n=0, summary=None, result=None)
    assert rc == -1 and "spec" in msg
    rc, msg = call(broken(n_rows=0), n=0, summary=None, result=None)
    assert rc == -1 and "summary" in msg
    rc, msg = call(broken(n_rows=0), n=0, result=None)
    assert rc == -1 and "result" in msg
    # n
    for n in (0, -5, 2 ** 31, 2 ** 40):
        rc, msg = call(broken(n_rows=0), n=n)
        assert rc == -1 and f"n = {n}" in msg
    # n_rows, n_q, replicates
    for bad in (0, 5, -1):
        rc, msg = call(broken(n_rows=bad, n_q=9))
        assert rc == -1 and "n_rows" in msg and str(bad) in msg
    for bad in (9, -1):
        rc, msg = call(broken(n_q=bad, replicates=0))
        assert rc == -1 and "n_q" in msg and str(bad) in msg
    for bad in (0, 65537, -1):
        spec = broken(replicates=bad)
        spec.rows[0] = 17
        rc, msg = call(spec)
        assert rc == -1 and "replicates" in msg and str(bad) in msg
    # rows: outside 0..16, listed twice, 16 without extra
    for bad in (17, -1):
        spec = broken()
        spec.rows[1] = bad
        rc, msg = call(spec)
        assert rc == -1 and "rows[1]" in msg and str(bad) in msg
    spec = broken()
    spec.rows[2] = spec.rows[0]
    rc, msg = call(spec)
    assert rc == -1 and "rows[2]" in msg and "twice" in msg
    spec = broken()
    spec.rows[1] = _abi.BOOT_ROW_EXTRA
    spec.q[0] = 2.0
    rc, msg = call(spec)
    assert rc == -1 and "extra" in msg
    # q, then level
    for bad in (-0.01, 1.01, float("nan")):
        spec = broken()
        spec.q[3] = bad
        rc, msg = call(spec)
        assert rc == -1 and "q[3]" in msg
    for bad in (0.0, 1.0, -0.5, float("nan")):
        spec = defaults(lib)
        spec.level = bad
        rc, msg = call(spec)
        assert rc == -1 and "level" in msg
    # everything in order, at the limits: only the context is left
    spec = defaults(lib)
    spec.n_rows, spec.n_q, spec.replicates, spec.level, spec.seed = 4, 8, 65536, 0.5, 2 ** 64 - 1
    spec.rows[:4] = [15, 0, 16, 7]
    spec.q[:8] = [0.0, 1.0, 0.5, 0.25, 0.75, 0.1, 0.9, 0.99]
    rc, msg = call(spec, n=2 ** 31 - 1, extra=DUMMY, rep=DUMMY)
    assert rc == -1 and "ctx" in msg
    spec = defaults(lib)
    spec.n_rows, spec.n_q, spec.replicates = 1, 0, 1
    rc, msg = call(spec, n=1)
    assert rc == -1 and "ctx" in msg


@pytest.mark.parametrize("m", [1, 2, 3, 5, 9, 255, 256, 257, 65537, 2 ** 31 - 1])
def test_bootstrap_indices_equal_the_reference_recipe(lib, m):
    """Whole replicates where they are small, windows with an odd `first` and a `count` that ends inside a pair everywhere."""
    for seed, b in ((0, 0), (1234, 7), (2 ** 64 - 1, 65535), (0xDEADBEEF12345678, 1999)):
        if m <= 65537:
            got = analysis.bootstrap_indices(seed, b, m)
            assert got.dtype == np.int64 and got.shape == (m,)
            assert np.array_equal(got, philox_ref.indices(seed, b, m))
            assert got.min() >= 0 and got.max() < m
        windows = {(0, min(m, 1)), (1 % m, min(m - 1 % m, 4)), (max(m - 3, 0), min(m, 3)), (max(m - 1, 0), 1), (m, 0),
                   (m // 2 | 1 if m > 2 else 0, min(m - (m // 2 | 1 if m > 2 else 0), 1001))}
        for first, count in windows:
            got = analysis.bootstrap_indices(seed, b, m, first=first, count=count)
            assert np.array_equal(got, philox_ref.indices(seed, b, m, first, count)), (first, count)
            assert got.shape == (count,) and (count == 0 or (got.min() >= 0 and got.max() < m))
    if m == 1:
        assert not analysis.bootstrap_indices(99, 3, 1).any()
    if m == 5:
        assert analysis.bootstrap_indices(0, 0, 5).tolist() == [4, 3, 1, 0, 1]
    if m == 9:
        assert analysis.bootstrap_indices(1234, 7, 9).tolist() == [1, 1, 6, 0, 1, 3, 6, 8, 0]


def test_bootstrap_indices_refuses_bad_arguments(lib):
    out = (C.c_int64 * 8)()

    def call(seed=0, replicate=0, m=8, first=0, count=8, buf=out):
        rc = lib.erpl_mc_bootstrap_indices(seed, replicate, m, first, count, buf)
        return rc, lib.erpl_mc_last_error().decode()

    assert call()[0] == 0
    rc, msg = call(buf=None)
    assert rc == -1 and "out" in msg
    for bad in (0, -1, 2 ** 31):
        rc, msg = call(m=bad, count=0)
        assert rc == -1 and "m = " in msg
    rc, msg = call(first=-1, count=1)
    assert rc == -1 and "first" in msg
    rc, msg = call(first=1, count=8)
    assert rc == -1 and "first + count" in msg
    rc, msg = call(first=9, count=0)
    assert rc == -1 and "first + count" in msg
    rc, msg = call(count=-1)
    assert rc == -1 and "count" in msg
    rc, msg = call(replicate=-1)
    assert rc == -1 and "replicate" in msg


def test_engine_bootstrap_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.bootstrap: the refusal is on the host, before the library is called."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.bootstrap(eng, torch.zeros((16, 4), dtype=torch.float64))
