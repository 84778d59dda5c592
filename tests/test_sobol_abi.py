"""erpl_mc_sobol and its defaults at the C boundary, as far as it goes without a GPU: struct layouts against gcc, the defaults,
every argument check (they come before any device work, in the order the header lists, and look at the context last: a NULL
context and a dummy pointer that is never dereferenced show them all), and the yardstick itself - the NumPy estimators of
sobol_ref, which the device tests compare against, recover the known indices of the Ishigami function."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import sobol_ref
from erpl_monte_carlo_sim_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = H.DUMMY

STRUCTS = (("erpl_sobol_spec", "ErplSobolSpec"), ("erpl_boot_stat", "ErplBootStat"), ("erpl_sobol_row", "ErplSobolRow"),
           ("erpl_sobol", "ErplSobol"))
MACROS = (("ERPL_SOBOL_MAX_FACTORS", _abi.SOBOL_MAX_FACTORS), ("ERPL_SOBOL_MAX_ROWS", _abi.SOBOL_MAX_ROWS),
          ("ERPL_SOBOL_ROW_EXTRA", _abi.SOBOL_ROW_EXTRA), ("ERPL_SOBOL_MAX_REPLICATES", _abi.SOBOL_MAX_REPLICATES),
          ("ERPL_SOBOL_MAX_STATS", _abi.SOBOL_MAX_STATS))


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and the offset of EVERY field of the four ctypes mirrors, and the five macros == what gcc sees."""
    H.check_struct_layouts(tmp_path, STRUCTS, MACROS)
    assert (_abi.SOBOL_MAX_FACTORS, _abi.SOBOL_MAX_ROWS, _abi.SOBOL_ROW_EXTRA, _abi.SOBOL_MAX_REPLICATES,
            _abi.SOBOL_MAX_STATS) == (32, 4, 16, 65536, 264)
    assert _abi.SOBOL_ROW_EXTRA == _abi.BOOT_ROW_EXTRA == _abi.SUMMARY_DIM and _abi.ABI_VERSION == 4
    # mean, variance, first[], total[] lie one behind the other: the host fills them as one run of erpl_boot_stat
    r, s = _abi.ErplSobolRow, C.sizeof(_abi.ErplBootStat)
    assert (r.variance.offset - r.mean.offset, r.first.offset - r.mean.offset, r.total.offset - r.mean.offset) == (s, 2 * s, 34 * s)


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_sobol_defaults", "erpl_mc_sobol"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def defaults(lib):
    spec = _abi.ErplSobolSpec()
    assert lib.erpl_mc_sobol_defaults(C.byref(spec)) == 0
    return spec


def test_defaults_are_exact(lib):
    spec = _abi.ErplSobolSpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_sobol_defaults(C.byref(spec)) == 0
    assert spec.n_rows == 3 and list(spec.rows) == [_abi.SUM_FIRST_APOGEE_ALT, _abi.SUM_FIRST_APOGEE_TIME,
                                                    _abi.SUM_RAIL_EXIT_SPEED, 0]
    assert spec.n_factors == 0 and spec.replicates == 1000 and spec.level == 0.95 and spec.seed == 0 and spec.reserved == 0
    assert lib.erpl_mc_sobol_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_argument_checks_come_before_any_device_work_in_the_documented_order(lib):
    res = _abi.ErplSobol()

    def call(spec, n_base=8, ld=None, summary=DUMMY, extra=None, result=res, rep=None):
        if ld is None:
            ld = 34 * max(n_base, 0)
        rc = lib.erpl_mc_sobol(None, summary, extra, None, n_base, ld, C.byref(spec) if spec is not None else None,
                               C.byref(result) if result is not None else None, rep, None)
        return rc, lib.erpl_mc_last_error().decode()

    def broken(**fields):
        """A spec with EVERY later check failing too: the earlier one has to be the one reported."""
        spec = defaults(lib)
        spec.n_factors, spec.level = 3, 1.0
        for k, v in fields.items():
            setattr(spec, k, v)
        return spec

    # 1. NULL spec, summary, result - in this order, whatever else is wrong
    rc, msg = call(None, n_base=0, summary=None, result=None)
    assert rc == -1 and "spec" in msg
    rc, msg = call(broken(n_factors=0), n_base=0, summary=None, result=None)
    assert rc == -1 and "summary" in msg
    rc, msg = call(broken(n_factors=0), n_base=0, result=None)
    assert rc == -1 and "result" in msg
    # 2. n_base
    for n in (0, -5):
        rc, msg = call(broken(n_factors=0), n_base=n)
        assert rc == -1 and f"n_base = {n}" in msg
    # 3. n_factors
    for bad in (0, 33, -1):
        rc, msg = call(broken(n_factors=bad, n_rows=0), n_base=2 ** 40, ld=0)
        assert rc == -1 and "n_factors" in msg and str(bad) in msg
    # 4. (n_factors + 2) * n_base >= 2^31: the first n_base that is too large, for k = 1, 3 and 32
    for k in (1, 3, 32):
        most = (2 ** 31 - 1) // (k + 2)
        rc, msg = call(broken(n_factors=k, n_rows=0), n_base=most + 1, ld=0)
        assert rc == -1 and "2^31" in msg and "n_base" in msg
        rc, msg = call(broken(n_factors=k, n_rows=0), n_base=most, ld=0)       # fits: the next check speaks
        assert rc == -1 and "ld = 0" in msg
    rc, msg = call(broken(n_rows=0), n_base=2 ** 62, ld=0)
    assert rc == -1 and "2^31" in msg
    # 5. ld
    rc, msg = call(broken(n_rows=0), n_base=8, ld=39)
    assert rc == -1 and "ld = 39" in msg and "40" in msg
    # 6. n_rows
    for bad in (0, 5, -1):
        spec = broken(n_rows=bad, replicates=-1)
        spec.rows[0] = 17
        rc, msg = call(spec, ld=40)
        assert rc == -1 and "n_rows" in msg and str(bad) in msg
    # 7. rows: outside 0..16, listed twice
    for bad in (17, -1):
        spec = broken(replicates=-1)
        spec.rows[1] = bad
        rc, msg = call(spec)
        assert rc == -1 and "rows[1]" in msg and str(bad) in msg
    spec = broken(replicates=-1)
    spec.rows[2] = spec.rows[0]
    rc, msg = call(spec)
    assert rc == -1 and "rows[2]" in msg and "twice" in msg
    # 8. row 16 without extra
    spec = broken(replicates=-1)
    spec.rows[1] = _abi.SOBOL_ROW_EXTRA
    rc, msg = call(spec)
    assert rc == -1 and "extra" in msg
    # 9. replicates
    for bad in (65537, -1):
        rc, msg = call(broken(replicates=bad), rep=DUMMY)
        assert rc == -1 and "replicates" in msg and str(bad) in msg
    # 10. replicates_out with replicates == 0 (level is not looked at then)
    rc, msg = call(broken(replicates=0), rep=DUMMY)
    assert rc == -1 and "replicates_out" in msg
    rc, msg = call(broken(replicates=0))
    assert rc == -1 and "ctx" in msg
    # 11. level
    for bad in (0.0, 1.0, -0.5, float("nan")):
        spec = defaults(lib)
        spec.n_factors, spec.level = 3, bad
        rc, msg = call(spec)
        assert rc == -1 and "level" in msg
    # 12. everything in order, at the limits: only the context is left
    spec = defaults(lib)
    spec.n_factors, spec.n_rows, spec.replicates, spec.level, spec.seed = 32, 4, 65536, 0.5, 2 ** 64 - 1
    spec.rows[:4] = [15, 0, 16, 7]
    most = (2 ** 31 - 1) // 34
    rc, msg = call(spec, n_base=most, ld=34 * most, extra=DUMMY, rep=DUMMY)
    assert rc == -1 and "ctx" in msg
    spec = defaults(lib)
    spec.n_factors, spec.n_rows, spec.replicates = 1, 1, 0
    rc, msg = call(spec, n_base=1, ld=3)
    assert rc == -1 and "ctx" in msg


def test_engine_sobol_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.sobol: the refusal is on the host, before the library is called."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.sobol(eng, torch.zeros((16, 12), dtype=torch.float64), 4, 1)


def test_the_numpy_yardstick_recovers_the_ishigami_indices():
    """Ishigami (a = 7, b = 0.1): S1 = 0.3139, 0.4424, 0 and ST = 0.5576, 0.4424, 0.2437.  n_base = 16 384 from
    default_rng(2024); every index within 0.03 of the truth - about 2.5 bootstrap standard errors at this size (the
    largest error is 0.0085 at this seed and 0.018 over the seeds 0..19)."""
    Y = sobol_ref.ishigami_design()
    assert Y.shape == (5, 16384)
    f0, V, S1, ST = sobol_ref.estimate(Y)
    err = np.abs(np.concatenate([S1 - sobol_ref.ISHIGAMI_S1, ST - sobol_ref.ISHIGAMI_ST]))
    print(f"Ishigami: S1 {S1}, ST {ST}, largest error {err.max():.4f}")
    assert np.all(err <= 0.03)
    # mean a / 2 and variance a^2 / 8 + b pi^4 / 5 + b^2 pi^8 / 18 + 1 / 2, at five standard errors of 32 768 values
    var = 49.0 / 8 + 0.1 * np.pi ** 4 / 5 + 0.01 * np.pi ** 8 / 18 + 0.5
    assert abs(f0 - 3.5) <= 5 * np.sqrt(var / 32768) and abs(V / var - 1.0) <= 0.05
    # the estimators in double lie within their own rounding bounds of the long double evaluation
    assert sobol_ref.check((f0, V, S1, ST), Y) <= 1.0


def test_the_yardstick_on_exact_cases():
    rng = np.random.default_rng(7)
    ya, yb = rng.normal(size=1000), rng.normal(size=1000)
    f0, V, S1, ST = sobol_ref.estimate(np.vstack([ya, yb, ya, yb]))
    assert S1[0] == 0.0 and ST[0] == 0.0            # AB_0 is A: the factor does nothing
    assert abs(ST[1] - 1.0) < 0.1 and abs(S1[1] - ST[1]) < 0.1   # AB_1 is B: the factor is everything
    f0, V, S1, ST = sobol_ref.estimate(np.full((3, 10), 2.5))
    assert f0 == 2.5 and V == 0.0 and np.isnan(S1).all() and np.isnan(ST).all()
