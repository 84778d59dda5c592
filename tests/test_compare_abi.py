"""erpl_mc_compare, its defaults and erpl_mc_compare_labels at the C boundary, as far as it goes without a GPU: struct layouts
against gcc, the defaults, every argument check (they come before any device work, in the order the header lists, and look at
the context last: a NULL context and a dummy pointer that is never dereferenced show them all), the labels of a permutation
against their restatement through philox_ref, and the yardstick itself - compare_ref, which the device tests compare
against - against scipy.stats."""
import ctypes as C
import os

import numpy as np
import pytest

import compare_cases as cases
import compare_ref as ref
import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = H.DUMMY

STRUCTS = (("erpl_cmp_spec", "ErplCmpSpec"), ("erpl_cmp_test", "ErplCmpTest"), ("erpl_cmp_row", "ErplCmpRow"),
           ("erpl_compare", "ErplCompare"))
MACROS = (("ERPL_CMP_MAX_ROWS", _abi.CMP_MAX_ROWS), ("ERPL_CMP_ROW_EXTRA", _abi.CMP_ROW_EXTRA),
          ("ERPL_CMP_MAX_PERMUTATIONS", _abi.CMP_MAX_PERMUTATIONS), ("ERPL_CMP_ENERGY_MAX_POINTS", _abi.CMP_ENERGY_MAX_POINTS))


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and the offset of EVERY field of the four ctypes mirrors, and the four macros == what gcc sees."""
    H.check_struct_layouts(tmp_path, STRUCTS, MACROS)
    assert (_abi.CMP_MAX_ROWS, _abi.CMP_ROW_EXTRA, _abi.CMP_MAX_PERMUTATIONS) == (4, 16, 4096)
    assert _abi.CMP_ROW_EXTRA == _abi.BOOT_ROW_EXTRA == _abi.SUMMARY_DIM and _abi.ABI_VERSION == 4


def test_new_symbols_are_declared_exported_and_documented(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_compare_defaults", "erpl_mc_compare", "erpl_mc_compare_labels"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)
    section = hdr[hdr.index("Did two runs come from the same law"):hdr.index("#define ERPL_CMP_MAX_ROWS")]
    assert "THE LABEL CONTRACT" in section and "N^2" in section and "row_x = -1" in section


def defaults(lib):
    spec = _abi.ErplCmpSpec()
    assert lib.erpl_mc_compare_defaults(C.byref(spec)) == 0
    return spec


def test_defaults_are_exact(lib):
    spec = _abi.ErplCmpSpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_compare_defaults(C.byref(spec)) == 0
    assert spec.n_rows == 3 and list(spec.rows) == [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, 0]
    assert spec.n_q == 5 and list(spec.q) == [0.05, 0.25, 0.5, 0.75, 0.95, 0.0, 0.0, 0.0]
    assert (spec.row_x, spec.row_y, spec.permutations, spec.reserved) == (_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y, 999, 0)
    assert spec.level == 0.95 and spec.seed == 0
    again = defaults(lib)
    assert bytes(spec) == bytes(again)                     # every byte is written, padding included
    assert lib.erpl_mc_compare_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_argument_checks_come_before_any_device_work_in_the_documented_order(lib):
    res = _abi.ErplCompare()

    def call(spec, n_a=8, n_b=8, summary_a=DUMMY, summary_b=DUMMY, extra_a=None, extra_b=None, result=res, null=None):
        rc = lib.erpl_mc_compare(None, summary_a, None, n_a, summary_b, None, n_b, extra_a, extra_b,
                                 C.byref(spec) if spec is not None else None, C.byref(result) if result is not None else None,
                                 null, None)
        return rc, lib.erpl_mc_last_error().decode()

    def broken(**fields):
        """A spec in which EVERY check fails; `fields` repairs the earlier ones: the first one left has to be reported."""
        spec = defaults(lib)
        spec.n_rows, spec.n_q, spec.row_x, spec.row_y, spec.permutations, spec.level = 0, 9, 16, 16, -1, 1.0
        spec.rows[:4] = [17, 17, 16, -1]
        spec.q[0] = 1.5
        for k, v in fields.items():
            if k == "rows":
                spec.rows[:len(v)] = v
            elif k == "q0":
                spec.q[0] = v
            else:
                setattr(spec, k, v)
        return spec

    # 1. NULL spec, summary_a, summary_b, result - in this order, whatever else is wrong
    rc, msg = call(None, n_a=0, n_b=0, summary_a=None, summary_b=None, result=None)
    assert rc == -1 and "spec" in msg
    rc, msg = call(broken(), n_a=0, n_b=0, summary_a=None, summary_b=None, result=None)
    assert rc == -1 and "summary_a" in msg
    rc, msg = call(broken(), n_a=0, n_b=0, summary_b=None, result=None)
    assert rc == -1 and "summary_b" in msg
    rc, msg = call(broken(), n_a=0, n_b=0, result=None)
    assert rc == -1 and "result" in msg
    # 2. n_a, then n_b
    for n in (0, -5, 2 ** 31, 2 ** 40):
        rc, msg = call(broken(), n_a=n, n_b=0)
        assert rc == -1 and f"n_a = {n}" in msg
        rc, msg = call(broken(), n_a=2 ** 31 - 1, n_b=n)
        assert rc == -1 and f"n_b = {n}" in msg
    # 3. n_rows
    for bad in (0, 5, -1):
        rc, msg = call(broken(n_rows=bad), n_a=2 ** 31 - 1, n_b=2 ** 31 - 1)
        assert rc == -1 and "n_rows" in msg and str(bad) in msg
    # 4. rows: outside 0..16, listed twice
    for bad in (17, -1):
        rc, msg = call(broken(n_rows=4, rows=[0, bad, 16, 16]))
        assert rc == -1 and "rows[1]" in msg and str(bad) in msg
    rc, msg = call(broken(n_rows=4, rows=[3, 16, 3, 16]))
    assert rc == -1 and "rows[2]" in msg and "twice" in msg
    # 5. row 16 without extra_a, then without extra_b
    rc, msg = call(broken(n_rows=2, rows=[3, 16]))
    assert rc == -1 and "extra_a" in msg
    rc, msg = call(broken(n_rows=2, rows=[3, 16]), extra_a=DUMMY)
    assert rc == -1 and "extra_b" in msg
    good = dict(n_rows=2, rows=[3, 16])
    both = dict(extra_a=DUMMY, extra_b=DUMMY)
    # 6. n_q, q
    for bad in (9, -1):
        rc, msg = call(broken(n_q=bad, **good), **both)
        assert rc == -1 and "n_q" in msg and str(bad) in msg
    for bad in (1.5, -0.1, float("nan")):
        rc, msg = call(broken(n_q=8, q0=bad, **good), **both)
        assert rc == -1 and "q[0]" in msg
    good.update(n_q=8, q0=1.0)
    # 7. row_x / row_y (looked at only when row_x >= 0)
    rc, msg = call(broken(**good), **both)
    assert rc == -1 and "row_x" in msg and "16" in msg
    rc, msg = call(broken(row_x=15, **good), **both)
    assert rc == -1 and "row_y" in msg and "16" in msg
    rc, msg = call(broken(row_x=15, row_y=15, **good), **both)
    assert rc == -1 and "row_y" in msg and "twice" in msg
    rc, msg = call(broken(row_x=-1, **good), **both)
    assert rc == -1 and "permutations" in msg
    # 8. permutations
    for bad in (-1, 4097):
        rc, msg = call(broken(row_x=0, row_y=15, permutations=bad, **good), null=DUMMY, **both)
        assert rc == -1 and "permutations" in msg and str(bad) in msg
    # 9. null_out with permutations == 0 (level is not looked at then)
    rc, msg = call(broken(row_x=-1, permutations=0, **good), null=DUMMY, **both)
    assert rc == -1 and "null_out" in msg
    rc, msg = call(broken(row_x=-7, permutations=0, **good), **both)
    assert rc == -1 and "ctx" in msg
    # 10. level
    for bad in (0.0, 1.0, -0.5, float("nan")):
        rc, msg = call(broken(row_x=-1, permutations=1, level=bad, **good), **both)
        assert rc == -1 and "level" in msg
    # 11. everything in order, at the limits: only the context is left
    spec = defaults(lib)
    spec.n_rows, spec.n_q, spec.row_x, spec.row_y, spec.permutations, spec.level, spec.seed = 4, 8, 15, 0, 4096, 0.5, 2 ** 64 - 1
    spec.rows[:4] = [15, 0, 16, 7]
    rc, msg = call(spec, n_a=2 ** 31 - 1, n_b=1, null=DUMMY, **both)
    assert rc == -1 and "ctx" in msg
    spec = defaults(lib)
    spec.n_rows, spec.n_q, spec.permutations = 1, 0, 0
    rc, msg = call(spec, n_a=1, n_b=2 ** 31 - 1)
    assert rc == -1 and "ctx" in msg


def test_engine_compare_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.compare: the refusal is on the host, before the library is called."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.compare(eng, torch.zeros((16, 12), dtype=torch.float64), torch.zeros((16, 9), dtype=torch.float64))


# ---------------------------------------------------------------------------------- the labels
@pytest.mark.parametrize("m_a, m_b", [(1, 1), (1, 6), (6, 1), (128, 129), (700, 325), (1500, 1000)])
def test_labels_have_m_a_ones_and_equal_the_restatement(m_a, m_b):
    seen = []
    for seed, p in ((0, 0), (0, 1), (2 ** 64 - 1, 0), (12345678901234567, 4095), (7, 2 ** 32 - 1)):
        got = analysis.permutation_labels(seed, p, m_a, m_b)
        assert got.dtype == bool and got.shape == (m_a + m_b,) and int(got.sum()) == m_a
        assert np.array_equal(got, ref.labels(seed, p, m_a, m_b)), (seed, p)
        seen.append(got)
    if m_a + m_b > 64:                                      # different permutations and different seeds differ
        assert all(not np.array_equal(seen[i], seen[j]) for i in range(5) for j in range(i))


def test_labels_at_the_edges(lib):
    assert analysis.permutation_labels(3, 5, 0, 9).sum() == 0 and analysis.permutation_labels(3, 5, 0, 9).shape == (9,)
    assert analysis.permutation_labels(3, 5, 9, 0).all()
    assert list(analysis.permutation_labels(3, 5, 1, 0)) == [True] and list(analysis.permutation_labels(3, 5, 0, 1)) == [False]
    out = (C.c_uint8 * 4)()
    for args, word in (((0, 0, 0, 0), "m_a + m_b"), ((0, 0, -1, 3), "m_a"), ((0, 0, 3, -1), "m_b"), ((0, -1, 2, 2), "permutation"),
                       ((0, 2 ** 32, 2, 2), "permutation"), ((0, 0, 2 ** 31, 2 ** 31), "m_a + m_b")):
        assert lib.erpl_mc_compare_labels(*args, out) == -1 and word in lib.erpl_mc_last_error().decode(), args
    assert lib.erpl_mc_compare_labels(0, 0, 2, 2, None) == -1 and "out" in lib.erpl_mc_last_error().decode()


def test_labels_break_equal_keys_by_index():
    """The rule behind a tie of two 64-bit keys, which no seed will show: side A is the smallest (key, i) PAIRS."""
    key = np.array([5, 3, 5, 3, 9], dtype=np.uint64)
    order = np.lexsort((np.arange(5), key))
    assert list(order[:3]) == [1, 3, 0]                     # of the two fives the one with the smaller index


# ---------------------------------------------------------------------------------- the yardstick against scipy
def samples(kind, m_a, m_b, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=m_a), rng.normal(0.2, 1.3, size=m_b)
    if kind == "tied":
        a, b = np.round(a, 1), np.round(b, 1)
    return a, b


@pytest.mark.parametrize("kind", ["continuous", "tied"])
@pytest.mark.parametrize("m_a, m_b", [(2, 2), (5, 300), (257, 255), (1500, 1000)])     # scipy wants two per sample
def test_the_yardstick_against_scipy(kind, m_a, m_b):
    stats = pytest.importorskip("scipy.stats")
    a, b = samples(kind, m_a, m_b, 17 * m_a + m_b)
    r = ref.rank_stats(ref.Ranked(np.r_[a, b]), ref.identity(m_a, m_b))
    # K against a brute-force ECDF at every pooled value, in integers
    pooled = np.unique(np.r_[a, b])
    ca = np.searchsorted(np.sort(a), pooled, side="right")
    cb = np.searchsorted(np.sort(b), pooled, side="right")
    v = m_b * ca - m_a * cb
    assert r["K"] == int(np.abs(v).max())
    first = int(np.argmax(np.abs(v)))
    assert r["value"] == pooled[first] and r["sign"] == int(np.sign(v[first]))
    # scipy subtracts two rounded distribution functions (values up to 1): its D carries up to one ulp OF THEM, 2^-52, whatever
    # the size of D; K / (m_a m_b) is the correctly rounded quotient of the exact integers
    d = stats.ks_2samp(a, b, method="asymp").statistic
    assert abs(r["D"] - d) <= np.spacing(1.0), (r["D"], d)
    u = stats.mannwhitneyu(a, b, method="asymptotic").statistic
    assert r["U2"] == int(round(2 * u)) and 2 * u == r["U2"]
    t = stats.cramervonmises_2samp(a, b, method="asymptotic").statistic
    assert abs(float(r["T"]) - t) <= 1e-12 * abs(t), (float(r["T"]), t)
    assert abs(r["T64"] - float(r["T"])) <= 1e-10 * max(abs(t), 1.0)


def test_the_yardstick_energy_forms_agree():
    """2 d_ab - d_aa - d_bb == - sum_i sum_j w_i w_j |z_i - z_j| with w = 1 / m_a on A, - 1 / m_b on B, and it is 0 for a cloud
    against itself."""
    rng = np.random.default_rng(4)
    xa, ya, xb, yb = rng.normal(size=40), rng.normal(size=40), rng.normal(0.5, 1, 25), rng.normal(size=25)
    cl = ref.Cloud(np.r_[xa, xb], np.r_[ya, yb])
    lab = ref.identity(40, 25)
    e = ref.energy_stats(cl, lab)
    w = np.where(lab, ref.LD(1) / 40, -ref.LD(1) / 25)
    assert abs(e["E"] + w @ cl.d @ w) <= 1e-17 and e["E"] > 0 and abs(e["E64"] - float(e["E"])) <= 1e-13
    same = ref.energy_stats(ref.Cloud(np.r_[xa, xa], np.r_[ya, ya]), ref.identity(40, 40))
    assert abs(same["E"]) <= 1e-17


def decide(name):
    """The p-values of the three rank tests of x and y and of the energy test, by the yardstick with its own labels (the energy
    statistic in plain float64: a decision, not a measurement)."""
    xa, ya, xb, yb = cases.law(name)
    m_a, m_b = len(xa), len(xb)
    labs = [ref.identity(m_a, m_b)] + [ref.labels(cases.DECISION_SEED, p, m_a, m_b) for p in range(cases.DECISION_P)]
    p = {}
    for row, (a, b) in (("x", (xa, xb)), ("y", (ya, yb))):
        rk = ref.Ranked(np.r_[a, b])
        st = [ref.rank_stats(rk, lab) for lab in labs]
        p[row] = {"ks": ref.null_summary([s["K"] for s in st[1:]], st[0]["K"], 0.95)["p"],
                  "mw": ref.null_summary([s["mw"] for s in st[1:]], st[0]["mw"], 0.95)["p"],
                  "cvm": ref.null_summary([float(s["T"]) for s in st[1:]], float(st[0]["T"]), 0.95)["p"]}
    e = ref.energy_f64_all(ref.Cloud(np.r_[xa, xb], np.r_[ya, yb], exact=False), labs)
    p["energy"] = ref.null_summary(e[1:], e[0], 0.95)
    p["energy"]["E"] = float(e[0])
    return p


@pytest.mark.parametrize("name", ["same", "shift", "corr"])
def test_the_yardstick_decides_the_three_laws(name):
    """The cases of test_gpu_compare's decision test, decided by the yardstick alone, with clear margins: frozen seeds."""
    p = decide(name)
    print(name, p)
    lowest = 1.0 / (cases.DECISION_P + 1)
    ranks = [v for row in ("x", "y") for v in p[row].values()]
    if name == "same":
        assert min(ranks + [p["energy"]["p"]]) > 0.15
    elif name == "shift":
        assert set(p["x"].values()) == {lowest} and p["energy"]["p"] == lowest
    else:
        assert p["energy"]["p"] == lowest and p["energy"]["E"] > 5 * p["energy"]["hi"] and min(ranks) > 0.15
