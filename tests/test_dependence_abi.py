"""erpl_mc_dependence and its defaults at the C boundary, as far as it goes without a GPU: struct layouts against gcc, the
defaults, every argument check (they come before any device work, in the order the header lists, and look at the context
last: a NULL context and a dummy pointer that is never dereferenced show them all), and the yardstick itself - the NumPy
measures of dependence_ref, which the device tests compare against, on cases with exact answers and on the Ishigami
function."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import dependence_ref as ref
import helpers as H
from erpl_monte_carlo_sim_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = H.DUMMY

STRUCTS = (("erpl_dep_spec", "ErplDepSpec"), ("erpl_dep_measure", "ErplDepMeasure"), ("erpl_dep_pair", "ErplDepPair"),
           ("erpl_dependence", "ErplDependence"))
MACROS = (("ERPL_DEP_MAX_FACTORS", _abi.DEP_MAX_FACTORS), ("ERPL_DEP_MAX_ROWS", _abi.DEP_MAX_ROWS),
          ("ERPL_DEP_ROW_EXTRA", _abi.DEP_ROW_EXTRA), ("ERPL_DEP_MAX_CLASSES", _abi.DEP_MAX_CLASSES),
          ("ERPL_DEP_MAX_CELLS", _abi.DEP_MAX_CELLS), ("ERPL_DEP_MAX_SHIFTS", _abi.DEP_MAX_SHIFTS))


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and the offset of EVERY field of the four ctypes mirrors, and the six macros == what gcc sees."""
    H.check_struct_layouts(tmp_path, STRUCTS, MACROS)
    assert (_abi.DEP_MAX_FACTORS, _abi.DEP_MAX_ROWS, _abi.DEP_ROW_EXTRA, _abi.DEP_MAX_CLASSES, _abi.DEP_MAX_CELLS,
            _abi.DEP_MAX_SHIFTS) == (32, 4, 16, 64, 64, 4096)
    assert _abi.DEP_ROW_EXTRA == _abi.BOOT_ROW_EXTRA == _abi.SUMMARY_DIM and _abi.ABI_VERSION == 4


def test_new_symbols_are_declared_exported_and_documented(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_dependence_defaults", "erpl_mc_dependence"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)
    assert "pick-freeze" in hdr.lower()[hdr.index("ONE ordinary run"):hdr.index("#define ERPL_DEP_MAX_FACTORS")]


def defaults(lib):
    spec = _abi.ErplDepSpec()
    assert lib.erpl_mc_dependence_defaults(C.byref(spec)) == 0
    return spec


def test_defaults_are_exact(lib):
    spec = _abi.ErplDepSpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_dependence_defaults(C.byref(spec)) == 0
    assert spec.n_rows == 3 and list(spec.rows) == [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, 0]
    assert (spec.n_factors, spec.classes, spec.cells, spec.shifts, spec.reserved) == (0, 16, 16, 200, 0)
    assert spec.level == 0.95 and spec.seed == 0
    assert lib.erpl_mc_dependence_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_argument_checks_come_before_any_device_work_in_the_documented_order(lib):
    res = _abi.ErplDependence()

    def call(spec, n=8, factors=DUMMY, summary=DUMMY, extra=None, result=res, null=None):
        rc = lib.erpl_mc_dependence(None, factors, summary, extra, None, n, C.byref(spec) if spec is not None else None,
                                    C.byref(result) if result is not None else None, None, None, null, None)
        return rc, lib.erpl_mc_last_error().decode()

    def broken(**fields):
        """A spec in which EVERY check fails; `fields` repairs the earlier ones: the first one left has to be reported."""
        spec = defaults(lib)
        spec.n_factors, spec.n_rows, spec.classes, spec.cells, spec.shifts, spec.level = 0, 0, 1, 65, -1, 1.0
        spec.rows[:4] = [17, 17, 16, -1]
        for k, v in fields.items():
            if k == "rows":
                spec.rows[:len(v)] = v
            else:
                setattr(spec, k, v)
        return spec

    # 1. NULL spec, factors, summary, result - in this order, whatever else is wrong
    rc, msg = call(None, n=0, factors=None, summary=None, result=None)
    assert rc == -1 and "spec" in msg
    rc, msg = call(broken(), n=0, factors=None, summary=None, result=None)
    assert rc == -1 and "factors" in msg
    rc, msg = call(broken(), n=0, summary=None, result=None)
    assert rc == -1 and "summary" in msg
    rc, msg = call(broken(), n=0, result=None)
    assert rc == -1 and "result" in msg
    # 2. n
    for n in (0, -5, 2 ** 31, 2 ** 40):
        rc, msg = call(broken(), n=n)
        assert rc == -1 and f"n = {n}" in msg
    # 3. n_factors
    for bad in (0, 33, -1):
        rc, msg = call(broken(n_factors=bad), n=2 ** 31 - 1)
        assert rc == -1 and "n_factors" in msg and str(bad) in msg
    # 4. n_rows
    for bad in (0, 5, -1):
        rc, msg = call(broken(n_factors=32, n_rows=bad))
        assert rc == -1 and "n_rows" in msg and str(bad) in msg
    # 5. rows: outside 0..16, listed twice
    for bad in (17, -1):
        rc, msg = call(broken(n_factors=1, n_rows=4, rows=[0, bad, 16, 16]))
        assert rc == -1 and "rows[1]" in msg and str(bad) in msg
    rc, msg = call(broken(n_factors=1, n_rows=4, rows=[3, 16, 3, 16]))
    assert rc == -1 and "rows[2]" in msg and "twice" in msg
    # 6. row 16 without extra
    rc, msg = call(broken(n_factors=1, n_rows=2, rows=[3, 16]))
    assert rc == -1 and "extra" in msg
    good_rows = dict(n_factors=1, n_rows=2, rows=[3, 16])
    # 7. classes
    for bad in (1, 65, -1):
        rc, msg = call(broken(classes=bad, **good_rows), extra=DUMMY)
        assert rc == -1 and "classes" in msg and str(bad) in msg
    # 8. cells
    for bad in (1, 65, 0):
        rc, msg = call(broken(classes=2, cells=bad, **good_rows), extra=DUMMY)
        assert rc == -1 and "cells" in msg and str(bad) in msg
    # 9. shifts
    for bad in (-1, 4097):
        rc, msg = call(broken(classes=64, cells=2, shifts=bad, **good_rows), extra=DUMMY, null=DUMMY)
        assert rc == -1 and "shifts" in msg and str(bad) in msg
    # 10. null_out with shifts == 0 (level is not looked at then)
    rc, msg = call(broken(classes=64, cells=64, shifts=0, **good_rows), extra=DUMMY, null=DUMMY)
    assert rc == -1 and "null_out" in msg
    rc, msg = call(broken(classes=64, cells=64, shifts=0, **good_rows), extra=DUMMY)
    assert rc == -1 and "ctx" in msg
    # 11. level
    for bad in (0.0, 1.0, -0.5, float("nan")):
        rc, msg = call(broken(classes=16, cells=16, shifts=1, level=bad, **good_rows), extra=DUMMY)
        assert rc == -1 and "level" in msg
    # 12. everything in order, at the limits: only the context is left
    spec = defaults(lib)
    spec.n_factors, spec.n_rows, spec.classes, spec.cells, spec.shifts, spec.level, spec.seed = 32, 4, 64, 64, 4096, 0.5, 2 ** 64 - 1
    spec.rows[:4] = [15, 0, 16, 7]
    rc, msg = call(spec, n=2 ** 31 - 1, extra=DUMMY, null=DUMMY)
    assert rc == -1 and "ctx" in msg
    spec = defaults(lib)
    spec.n_factors, spec.n_rows, spec.classes, spec.cells, spec.shifts = 1, 1, 2, 2, 0
    rc, msg = call(spec, n=1)
    assert rc == -1 and "ctx" in msg


def test_engine_dependence_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.dependence: the refusal is on the host, before the library is called."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.dependence(eng, torch.zeros((2, 12), dtype=torch.float64), torch.zeros((16, 12), dtype=torch.float64))


# ---------------------------------------------------------------------------------- the yardstick on exact cases
@pytest.mark.parametrize("M, m", [(16, 1024), (3, 21), (64, 320)])
def test_yardstick_strictly_monotone_pair(M, m):
    """y = exp(x / m) of a permutation, M = H, M | m: a diagonal table.  delta_num = 2 m^2 (1 - 1 / M); ks_max = 1 - 1 / M,
    as the correctly rounded quotient (M - 1) / M that the integers give; mi = log M within 4 ulp of 1."""
    x = np.random.default_rng(M).permutation(m).astype(np.float64)
    out = ref.dependence(x, np.exp(x / m), classes=M, cells=M, shifts=0)
    assert np.array_equal(out["tables"][0, 0], np.eye(M, dtype=np.int64) * (m // M))
    assert out["delta_num"][0, 0] == 2 * m * m * (M - 1) // M
    assert out["delta"]["estimate"][0, 0] == (M - 1) / M
    assert out["ks_max"]["estimate"][0, 0] == (M - 1) / M
    assert abs(out["mi"]["estimate"][0, 0] - math.log(M)) <= 4 * 2.0 ** -52
    assert out["classes_used"][0, 0] == out["cells_used"][0, 0] == M
    assert 0.0 < out["eta2"][0, 0] < 1.0          # a share of the variance (about 1 - 1 / M^2 for a near-linear y)


def test_yardstick_constant_factor_with_both_zeros():
    """-0.0 ties with +0.0: one class, M div 2, and delta_num = 0, ks = 0, mi = 0.0 exactly; eta2 = 0, the others NaN."""
    rng = np.random.default_rng(3)
    x = np.where(rng.random(500) < 0.5, -0.0, 0.0)
    for M in (2, 7, 16):
        out = ref.dependence(x, rng.normal(size=500), classes=M, cells=5, shifts=3, seed=1)
        assert set(out["xc"][0]) == {M // 2} and out["classes_used"][0, 0] == 1
        assert out["delta_num"][0, 0] == 0
        for key in ref.MEASURES:
            assert out[key]["estimate"][0, 0] == 0.0 and not np.signbit(out[key]["estimate"][0, 0])
            assert np.all(out["null_values"][0, 0] == 0.0) and out[key]["exceed"][0, 0] == 3
        assert out["eta2"][0, 0] == 0.0 and np.isnan(out["eta2_adj"][0, 0]) and np.isnan(out["f_stat"][0, 0])


def test_yardstick_product_design_is_uniform():
    """xc = d mod M, yc = (d div M) mod H, m = 3 M H: every cell holds 3 and every measure is exactly 0."""
    M, Hc = 5, 7
    d = np.arange(3 * M * Hc)
    out = ref.dependence((d % M).astype(np.float64), ((d // M) % Hc).astype(np.float64), classes=M, cells=Hc, shifts=0)
    assert np.array_equal(out["xc"][0], d % M) and np.array_equal(out["yc"][0], (d // M) % Hc)
    assert np.all(out["tables"][0, 0] == 3) and out["delta_num"][0, 0] == 0
    for key in ref.MEASURES:
        assert out[key]["estimate"][0, 0] == 0.0
    assert out["eta2"][0, 0] == 0.0


def test_yardstick_heavy_ties_share_a_class():
    """Integers 0..4, m = 1001, M = 7: tied values share a class and two classes stay empty."""
    x = (np.arange(1001) % 5).astype(np.float64)
    y = np.random.default_rng(11).normal(size=1001) + x
    out = ref.dependence(x, y, classes=7, cells=4, shifts=0)
    xc = out["xc"][0]
    for v in range(5):
        assert len(set(xc[x == v])) == 1
    assert sorted(set(xc)) == [0, 2, 3, 4, 6] and out["classes_used"][0, 0] == 5
    cs = out["class_stats"][0, 0]
    assert list(cs[:, 0]) == [201, 0, 200, 200, 200, 0, 200] and np.isnan(cs[1, 1:]).all() and np.isnan(cs[5, 1:]).all()
    assert list(cs[[0, 2, 3, 4, 6], 3]) == list(cs[[0, 2, 3, 4, 6], 4]) == list(cs[[0, 2, 3, 4, 6], 5]) == [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def ishigami():
    x, y = ref.ishigami_case()
    return ref.dependence(x, y, classes=16, cells=16, shifts=200, level=0.95, seed=0)


def test_the_yardstick_on_the_ishigami_function(ishigami):
    """a = 7, b = 0.1, x uniform on (-pi, pi) plus a dummy, n = 16 384 from default_rng(2024), M = H = 16, P = 200.
    eta2_adj within 0.05 of the first-order indices (0.3139, 0.4424, 0, 0): a NumPy prototype of the class rule gave a
    largest error of 0.033 over the seeds 0..19 (the coarse classes).  delta of x1, x2, x3 clears its null_hi by 0.03 at
    least (prototype: smallest margins 0.18, 0.33, 0.049) - x3 is the case that matters: eta2 about 0, delta clearly above
    the band.  The dummy's null_mean of delta lies in 0.04..0.055 (prototype 0.0466), its estimate below null_hi + 0.01."""
    out = ishigami
    eta, d = out["eta2_adj"][0], out["delta"]
    print(f"Ishigami: eta2 {out['eta2'][0]}, eta2_adj {eta}")
    print(f"delta {d['estimate'][0]}, null_mean {d['null_mean'][0]}, null_hi {d['null_hi'][0]}, exceed {d['exceed'][0]}")
    for key in ("ks_max", "ks_median", "mi"):
        print(f"{key} {out[key]['estimate'][0]}, null_mean {out[key]['null_mean'][0]}, null_hi {out[key]['null_hi'][0]}")
    assert out["count"] == 16384
    assert np.all(np.abs(eta - np.array([0.3139, 0.4424, 0.0, 0.0])) <= 0.05)
    assert np.all(d["estimate"][0, :3] - d["null_hi"][0, :3] >= 0.03)
    assert 0.04 <= d["null_mean"][0, 3] <= 0.055
    assert d["estimate"][0, 3] < d["null_hi"][0, 3] + 0.01
    assert abs(out["eta2"][0, 2]) < 0.01 and d["exceed"][0, 2] == 0
