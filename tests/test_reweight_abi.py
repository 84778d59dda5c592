"""erpl_mc_reweight at the C boundary, no GPU: the struct mirrors, the defaults, erpl_mc_reweight_host against the NumPy
restatement (reweight_ref), the portable exp against math.exp, exact conditioning, NumPy's own weighted quantile, the law
itself on 64 designs, the closed-form ESS share, every refusal in the header's order, the host check program, law_change."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import design_cases as DC
import helpers as H
import reweight_cases as RC
import reweight_ref as R
from erpl_monte_carlo_sim_amd import _abi, analysis, models, sampling

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
DUMMY = H.DUMMY
ERR_INVALID = -1     # ERPL_ERR_INVALID
N, U = _abi.DESIGN_NORMAL, _abi.DESIGN_UNIFORM
NAMES = ("erpl_mc_reweight_defaults", "erpl_mc_reweight", "erpl_mc_reweight_host")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def host(case, **kw):
    return analysis.reweight_host(case["factors"], case["kinds"], case["law"], case["summary"], mask=case["mask"], rows=case["rows"],
                                  extra=case["extra"], thresholds=case["thresholds"], quantiles=case["quantiles"], want_weights=True, **kw)


# ------------------------------------------------------------------------------------------------ the boundary
def test_struct_layout_matches_the_c_compiler(tmp_path):
    H.check_struct_layouts(tmp_path, (("erpl_rw_spec", "ErplRwSpec"), ("erpl_rw_row_stats", "ErplRwRowStats"), ("erpl_reweight", "ErplReweight")),
                           (("ERPL_RW_MAX_LAW", _abi.RW_MAX_LAW), ("ERPL_RW_MAX_ROWS", _abi.RW_MAX_ROWS), ("ERPL_RW_ROW_EXTRA", _abi.RW_ROW_EXTRA),
                            ("ERPL_RW_MAX_THRESHOLDS", _abi.RW_MAX_THRESHOLDS), ("ERPL_RW_MAX_Q", _abi.RW_MAX_Q)))


def test_new_symbols_are_declared_exported_and_documented(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)
    assert _abi.ABI_VERSION == 4 and lib.erpl_mc_abi_version() == 4


def test_defaults_are_exact(lib):
    spec = _abi.ErplRwSpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_reweight_defaults(C.byref(spec)) == 0
    assert spec.n_law == 1 and spec.kind[0] == N and list(spec.kind[1:]) == [0] * 31 and spec.reserved == 0
    assert list(spec.mu) == [0.0] * 32 and list(spec.s) == [1.0] * 32 and list(spec.a) == [0.0] * 32 and list(spec.b) == [1.0] * 32
    assert spec.n_rows == 3 and list(spec.rows) == [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, 0]
    assert list(spec.n_thresholds) == [0] * 4 and all(v == 0.0 for row in spec.threshold for v in row)
    assert spec.n_q == 5 and list(spec.q) == [0.05, 0.25, 0.5, 0.75, 0.95, 0.0, 0.0, 0.0]
    assert lib.erpl_mc_reweight_defaults(None) == ERR_INVALID and b"spec" in lib.erpl_mc_last_error()


def test_the_host_check_program_passes(lib):
    exe = os.path.join(CSRC, "erpl_reweight_check")
    assert os.path.exists(exe), "erpl_reweight_check is built by `make all` (build())"
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("ok erpl_reweight_check") and "FAIL" not in res.stdout


def test_the_layout_of_the_workspace(lib):
    """work, then the log-weights and the weights the caller does not keep: every piece at a multiple of 256 bytes, an empty
    piece where the one before it ends rounded up, `need` the end of the last."""
    exe = os.path.join(CSRC, "erpl_stat_layout_table")
    ask = "rw 1000 0 0 5000\nrw 1000 1 0 5000\nrw 1000 0 1 5000\nrw 1 1 1 777\n"
    out = subprocess.run([exe], input=ask, capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [0, 5120, 5120 + 8192, 5120 + 8192 + 8000]
    assert [int(v) for v in out[1].split()] == [0, 5120, 5120, 5120 + 8000]
    assert [int(v) for v in out[2].split()] == [0, 5120, 5120 + 8192, 5120 + 8192]
    assert [int(v) for v in out[3].split()] == [0, 1024, 1024, 1024]


# ------------------------------------------------------------------------------------------------ the host twin against the restatement
@pytest.mark.parametrize("n", RC.SIZES)
@pytest.mark.parametrize("variant", RC.VARIANTS)
def test_host_twin_matches_the_restatement(lib, variant, n):
    case = RC.make_case(variant, n)
    got, want = host(case), RC.reference(case)
    RC.compare(got, want, f"{variant}-{n}")
    assert got["count"] + got["n_masked"] + got["n_non_finite"] + got["n_outside"] == n
    if n >= 63:
        assert got["count"] > 0 and got["max_w"] == 1 << got["Q"] and got["sum_w"] <= 1 << 62
    if variant == "mixed" and n >= 63:
        assert got["n_non_finite"] >= 5 and got["n_masked"] > 0 and got["n_outside"] > 0
        assert np.isnan(got["logw"][3]) and (np.isneginf(got["logw"]).sum() == got["n_outside"])


def test_a_strided_call_reads_its_own_columns_only(lib):
    case, wide = RC.make_case("mixed", 257), RC.make_case("mixed", 257, pad=7)
    assert wide["factors"].strides[0] == (257 + 7) * 8 and np.array_equal(RC.bits(case["summary"]), RC.bits(wide["summary"]))
    a, b = host(case), host(wide)
    RC.compare(b, a, "strided", scales=RC.mean_scales(case, a["weights"]))
    assert H.same_nested({k: v for k, v in a.items() if k not in ("logw", "weights")}, {k: v for k, v in b.items() if k not in ("logw", "weights")})


def test_a_support_of_one_column_and_an_empty_support(lib):
    n = 300
    rng = np.random.default_rng(3)
    summary = rng.normal(size=(_abi.SUMMARY_DIM, n))
    u = np.linspace(0.001, 0.999, n)[None, :].copy()
    one = dict(factors=u, kinds=[U], law=[(u[0, 137] - 1e-9, u[0, 137] + 1e-9)], summary=summary, mask=None, rows=None, extra=None,
               thresholds={_abi.SUM_RANGE: [summary[_abi.SUM_RANGE, 137] - 1.0, summary[_abi.SUM_RANGE, 137]]}, quantiles=(0.0, 0.5, 1.0))
    got = host(one)
    RC.compare(got, RC.reference(one), "one column")
    r = got["rows"][_abi.SUM_RANGE]
    assert got["count"] == 1 and got["n_outside"] == n - 1 and got["sum_w"] == got["max_w"] == 1 << 52 and got["ess"] == 1.0
    assert r["quantiles"] == [summary[_abi.SUM_RANGE, 137]] * 3 and r["mean"] == summary[_abi.SUM_RANGE, 137] and r["std"] == 0.0
    assert r["p"] == [1.0, 0.0] and r["p_se"] == [0.0, 0.0] and r["mean_se"] == 0.0
    empty = dict(one, law=[(0.9995, 1.0)])
    got = host(empty)
    RC.compare(got, RC.reference(empty), "empty")
    r = got["rows"][_abi.SUM_RANGE]
    assert got["count"] == 0 and got["n_outside"] == n and got["sum_w"] == 0 and got["max_w"] == 0 and r["exceed_w"] == [0, 0]
    assert all(math.isnan(v) for v in [got["ess"], got["sum_w2"], r["mean"], r["std"], r["mean_se"], r["min"], r["max"]] + r["quantiles"] + r["p"] + r["p_se"])
    assert not np.any(got["weights"]) and np.all(np.isneginf(got["logw"]))
    masked = dict(one, mask=np.ones(n, dtype=np.uint8))
    got = host(masked)
    assert got["count"] == 0 and got["n_masked"] == n and np.all(np.isnan(got["logw"]))


# ------------------------------------------------------------------------------------------------ the portable exp
def test_portable_exp_is_within_two_ulp_of_libm():
    """Measured here: at most 1.0 ulp on these 10^6 points (printed); the bar is that plus one ulp of margin for another libm."""
    rng = np.random.default_rng(17)
    x = np.concatenate([rng.uniform(-64.0, 0.0, 10 ** 6 - 4), [0.0, -64.0, -1e-300, -0.5 * math.log(2.0)]])
    got = R.rw_exp(x)
    want = np.array([math.exp(v) for v in x])
    err = np.abs(got - want) / H.ulp(want, np.float64)
    print(f"portable exp: at most {err.max():.3f} ulp from math.exp on {x.size} points of [-64, 0]")
    assert err.max() <= 2.0 and got.max() == 1.0 and R.rw_exp(np.array([0.0]))[0] == 1.0 and np.all(got > 0.0)
    assert np.array_equal(R.rw_exp(np.array([np.nextafter(-64.0, -np.inf), -1e9, -np.inf, np.nan])), np.zeros(4))


def test_the_library_uses_that_exp(lib):
    """One normal row with s = 1: l = z - 1 / 2 is spread over 60 units by z, and W = floor(2^Q e(l - l_max)) bit for bit."""
    n = 4001
    z = np.linspace(-30.0, 30.0, n)[None, :].copy()
    summary = np.zeros((_abi.SUMMARY_DIM, n))
    got = analysis.reweight_host(z, [N], [(1.0, 1.0)], summary, want_weights=True)
    l, Q = got["logw"], got["Q"]
    assert Q == 50 and np.allclose(l, z[0] - 0.5, rtol=0.0, atol=1e-12)
    assert np.array_equal(got["weights"], np.floor(np.ldexp(R.rw_exp(l - l.max()), Q)).astype(np.int64))
    assert got["weights"].max() == 1 << Q and np.all(np.diff(got["weights"]) >= 0)
    below = l - l.max() < -50.0 * math.log(2.0) - 1e-9                      # 2^50 e(d) < 1: the weight floors to 0
    assert got["n_zero"] == int((got["weights"] == 0).sum()) >= int(below.sum()) > 0 and np.all(got["weights"][~below][1:] > 0)


# ------------------------------------------------------------------------------------------------ exactness
def test_conditioning_is_exact(lib):
    """Only uniform rows change: every W of the support is 2^Q, and the integers and the quantiles are those of the subset."""
    n = 5000
    rng = np.random.default_rng(8)
    u = rng.uniform(size=(2, n))
    summary = np.round(rng.normal(size=(_abi.SUMMARY_DIM, n)) * 40.0) + 500.0
    qs, thr = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0), [450.0, 500.0, 530.0]
    got = analysis.reweight_host(u, [U, U], [(0.25, 0.75), (0.0, 0.5)], summary, rows=["range"], thresholds={"range": thr}, quantiles=qs,
                                 want_weights=True)
    sel = (u[0] >= 0.25) & (u[0] <= 0.75) & (u[1] <= 0.5)
    x = summary[_abi.SUM_RANGE][sel]
    Q = got["Q"]
    assert Q == 49 and got["count"] == int(sel.sum()) and got["n_outside"] == n - got["count"] and got["n_zero"] == 0
    assert np.array_equal(got["weights"], np.where(sel, 1 << Q, 0)) and got["sum_w"] == got["count"] << Q and got["ess"] == got["count"]
    r = got["rows"][_abi.SUM_RANGE]
    assert r["quantiles"] == [float(v) for v in np.quantile(x, qs, method="inverted_cdf")]
    assert r["exceed_w"] == [int((x > t).sum()) << Q for t in thr] and r["p"] == [float((x > t).sum()) / x.size for t in thr]
    assert math.isclose(got["ess_expected_share"], 0.25, rel_tol=1e-15) and r["min"] == x.min() and r["max"] == x.max()


def test_weighted_quantiles_are_numpys_own(lib):
    """np.quantile(x, q, weights=W, method='inverted_cdf') on the columns that carry weight; sum_w < 2^53, so NumPy's float64
    cumulative sum of the weights is exact."""
    n = 64
    z = np.linspace(-3.0, 3.0, n)[None, :].copy()
    rng = np.random.default_rng(21)
    summary = np.round(rng.normal(size=(_abi.SUMMARY_DIM, n)) * 3.0)          # ties
    qs = (0.01, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0)
    got = analysis.reweight_host(z, [N], [(2.5, 0.05)], summary, rows=["range", "impact_x"], quantiles=qs, want_weights=True)
    W = got["weights"]
    assert got["sum_w"] < 1 << 53 and (W > 0).sum() >= 8 and got["n_zero"] > 0
    for row in (_abi.SUM_RANGE, _abi.SUM_IMPACT_X):
        want = np.quantile(summary[row][W > 0], qs, weights=W[W > 0], method="inverted_cdf")
        assert got["rows"][row]["quantiles"] == [float(v) for v in want], row


def test_an_identity_law_is_the_plain_statistics(lib):
    n = 3001
    rng = np.random.default_rng(4)
    f = np.vstack([rng.normal(size=n), rng.uniform(size=n)])
    summary = rng.normal(size=(_abi.SUMMARY_DIM, n)) * 70.0 + 1000.0
    mask = (rng.uniform(size=n) < 0.2).astype(np.uint8)
    got = analysis.reweight_host(f, [N, U], [(0.0, 1.0), (0.0, 1.0)], summary, mask=mask, want_weights=True)
    assert got["ess"] == got["count"] == int((mask == 0).sum()) and got["ess_expected_share"] == 1.0
    assert np.array_equal(got["weights"], np.where(mask == 0, 1 << got["Q"], 0))
    for row in (_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME):
        x, r = summary[row][mask == 0], got["rows"][row]
        assert math.isclose(r["mean"], np.mean(x), rel_tol=1e-12) and math.isclose(r["std"], np.std(x), rel_tol=1e-12)
        assert math.isclose(r["mean_se"], np.std(x) / math.sqrt(x.size), rel_tol=1e-12)


# ------------------------------------------------------------------------------------------------ the law is right
LAW_KINDS, LAW = [N, N, N, U], [(0.3, 0.7), (0.0, 0.5), (-0.2, 1.1), (0.2, 0.6)]


@pytest.fixture(scope="module")
def law_runs(lib):
    """64 seeds of erpl_mc_design_host 'random' designs, n = 4096: y = 2 z0 + z1^2 - z2 + 3 u, whose mean under the target is
    2 * 0.3 + 0.25 + 0.2 + 3 * 0.4 = 2.25."""
    runs = []
    for seed in range(64):
        f = DC.host_design(lib, _abi.DESIGN_RANDOM, LAW_KINDS, 4096, seed=1000 + seed)
        summary = np.zeros((_abi.SUMMARY_DIM, 4096))
        summary[_abi.SUM_RANGE] = 2.0 * f[0] + f[1] * f[1] - f[2] + 3.0 * f[3]
        runs.append(analysis.reweight_host(f, LAW_KINDS, LAW, summary, rows=["range"], thresholds={"range": [3.0]}))
    return runs


def test_the_law_is_right(law_runs):
    """Measured with these designs: printed below (NumPy draws over 400 seeds gave a z-score spread of 1.004, maximum 3.08).
    The ESS share is taken of the FLOWN columns, count + n_outside (here all 4096): that is what 1 / prod E[w_r^2] is the
    expectation of - the uniform row's 1 / (b - a) is the share of the flown columns that fall inside the target range.
    Of `count` alone, the columns inside the support, the share would be 0.498, that of the three normal rows."""
    rows = [r["rows"][_abi.SUM_RANGE] for r in law_runs]
    z = np.array([(r["mean"] - 2.25) / r["mean_se"] for r in rows])
    p = np.array([r["p"][0] for r in rows])
    zp = np.array([(r["p"][0] - p.mean()) / r["p_se"][0] for r in rows])
    share = np.mean([r["ess"] / (r["count"] + r["n_outside"]) for r in law_runs])
    print(f"mean: z-scores std {z.std():.3f}, max {np.abs(z).max():.2f}; p(y > 3) = {p.mean():.4f}: z-scores std {zp.std():.3f}, "
          f"max {np.abs(zp).max():.2f}; mean p_se {np.mean([r['p_se'][0] for r in rows]):.5f} against a spread of {p.std():.5f}; "
          f"ess share {share:.4f} against {law_runs[0]['ess_expected_share']:.4f}")
    assert np.all(np.abs(z) <= 5.0) and 0.75 <= z.std() <= 1.25
    assert np.all(np.abs(zp) <= 5.0) and 0.75 <= zp.std() <= 1.25
    assert abs(share / law_runs[0]["ess_expected_share"] - 1.0) <= 0.05


def test_expected_ess_share_is_the_closed_form(lib):
    z = np.zeros((4, 8))
    u = np.full((1, 8), 0.5)
    summary = np.zeros((_abi.SUMMARY_DIM, 8))
    want = 1.0
    for mu, s in LAW[:3]:
        want *= math.exp(mu * mu / (2.0 - s * s)) / (s * math.sqrt(2.0 - s * s))
    want = 1.0 / (want / 0.4)
    got = analysis.reweight_host(np.vstack([z[:3], u]), LAW_KINDS, LAW, summary)["ess_expected_share"]
    assert math.isclose(got, want, rel_tol=1e-12) and math.isclose(got, 0.1993, rel_tol=2e-3)
    assert math.isclose(analysis.reweight_host(z[:1], [N], [(0.0, 0.5)], summary)["ess_expected_share"], 0.5 * math.sqrt(1.75), rel_tol=1e-12)
    for s in (math.sqrt(2.0), 1.5, 10.0):
        assert analysis.reweight_host(z[:1], [N], [(0.0, s)], summary)["ess_expected_share"] == 0.0
    assert analysis.reweight_host(z[:1], [N], [(0.0, 1.4)], summary)["ess_expected_share"] > 0.0


def test_warnings_of_the_finished_dict():
    base = {"count": 1000, "n_outside": 0, "sum_w": 1 << 60, "max_w": 1 << 52, "ess": 500.0, "ess_expected_share": 0.5, "rows": {_abi.SUM_RANGE: {}, _abi.RW_ROW_EXTRA: {}}}
    ok = analysis.finish_reweighted(dict(base))
    assert ok["warnings"] == [] and ok["ess_share"] == 0.5 and ok["max_weight_share"] == 2.0 ** -8 and ok["row_names"] == ["range", "extra"]
    assert "infinite" in analysis.finish_reweighted(dict(base, ess_expected_share=0.0))["warnings"][0]
    assert analysis.finish_reweighted(dict(base, count=600, n_outside=400))["ess_share"] == 0.5
    assert "below 100" in analysis.finish_reweighted(dict(base, ess=99.0))["warnings"][0]
    assert "of the weight" in analysis.finish_reweighted(dict(base, max_w=1 << 58))["warnings"][0]
    e = analysis.finish_reweighted(dict(base, count=0, sum_w=0, max_w=0, ess=math.nan))
    assert "empty" in e["warnings"][0] and math.isnan(e["ess_share"]) and math.isnan(e["max_weight_share"])


# ------------------------------------------------------------------------------------------------ every refusal
def refusals():
    """(keyword overrides, a word of the message), in the order of the header."""
    spec = lambda **kw: {"spec_fields": kw}
    return [({"spec": None}, "spec"), (spec(n_law=0), "n_law"), (spec(n_law=33), "n_law"),
            (spec(kind=(1, 7)), "kind[1]"), (spec(mu=(0, math.inf)), "mu[0]"), (spec(mu=(0, math.nan)), "mu[0]"), (spec(s=(0, 0.0)), "s[0]"),
            (spec(s=(0, -1.0)), "s[0]"), (spec(s=(0, math.inf)), "s[0]"), (spec(s=(0, math.nan)), "s[0]"),
            (spec(a=(1, -0.1)), "a[1]"), (spec(b=(1, 1.5)), "a[1]"), (spec(a=(1, 0.5), b=(1, 0.5)), "a[1]"), (spec(a=(1, math.nan)), "a[1]"),
            (spec(n_rows=0), "n_rows"), (spec(n_rows=5), "n_rows"), (spec(rows=(1, 17)), "rows[1]"), (spec(rows=(0, -1)), "rows[0]"),
            (spec(rows=(1, _abi.SUM_APOGEE_ALT)), "twice"), ({"extra": None, "spec_fields": {"rows": (2, 16)}}, "extra"),
            (spec(n_thresholds=(1, 9)), "n_thresholds[1]"), (spec(n_thresholds=(0, -1)), "n_thresholds[0]"),
            ({"spec_fields": {"n_thresholds": (2, 2)}, "nan_threshold": (2, 1)}, "threshold[2][1]"),
            (spec(n_q=9), "n_q"), (spec(n_q=-1), "n_q"), (spec(q=(2, 1.5)), "q[2]"), (spec(q=(0, math.nan)), "q[0]"), (spec(q=(4, -0.1)), "q[4]"),
            ({"factors": None}, "factors"), ({"summary": None}, "summary"), ({"result": None}, "result"),
            ({"n": 0}, "n ="), ({"n": -3}, "n ="), ({"n": 2 ** 31}, "n ="), ({"ld": 7}, "ld ="), ({"ld_s": 7}, "ld_s ="), ({"ctx": None}, "ctx")]


def call_entry(lib, host, kw):
    """One call with good arguments (host pointers that are never dereferenced: every refusal comes first) but for `kw`."""
    kw = dict(kw)
    ctx = kw.pop("ctx", DUMMY)
    spec = _abi.ErplRwSpec()
    assert lib.erpl_mc_reweight_defaults(C.byref(spec)) == 0
    spec.n_law, spec.kind[0], spec.kind[1] = 2, N, U
    for k, v in kw.pop("spec_fields", {}).items():
        if isinstance(v, tuple):
            getattr(spec, k)[v[0]] = v[1]
        else:
            setattr(spec, k, v)
    if "nan_threshold" in kw:
        j, k = kw.pop("nan_threshold")
        spec.threshold[j][k] = math.nan
    sp = None if "spec" in kw and kw.pop("spec") is None else C.byref(spec)
    arg = lambda k: kw.pop(k) if k in kw else DUMMY
    res = _abi.ErplReweight()
    result = None if "result" in kw and kw.pop("result") is None else C.byref(res)
    args = [sp, arg("factors"), kw.pop("ld", 8), arg("summary"), kw.pop("ld_s", 8), arg("extra"), None, kw.pop("n", 8), result, None, None]
    assert not kw, kw
    fn = lib.erpl_mc_reweight_host if host else lib.erpl_mc_reweight
    return fn(*(([] if host else [ctx]) + args + ([] if host else [None])))


@pytest.mark.parametrize("kw,word", refusals(), ids=[f"{i}-{w}" for i, (_, w) in enumerate(refusals())])
def test_every_refusal_names_its_argument(lib, kw, word):
    for host_call in (False, True):
        if "ctx" in kw and host_call:
            continue
        assert call_entry(lib, host_call, kw) == ERR_INVALID, (kw, host_call)
        assert word.encode() in lib.erpl_mc_last_error(), (kw, lib.erpl_mc_last_error())


def test_refusals_come_in_the_order_of_the_header(lib):
    """Two faults at once: the one the header lists first is reported."""
    f = lambda **kw: {"spec_fields": kw}
    pairs = [(f(n_law=0, kind=(0, 7)), "n_law"), (f(mu=(0, math.inf), kind=(1, 7)), "mu[0]"), (f(kind=(0, 7), a=(1, 2.0)), "kind[0]"),
             (f(s=(0, 0.0), n_rows=0), "s[0]"), (f(a=(1, 0.7), b=(1, 0.2), n_rows=9), "a[1]"), (f(n_rows=5, rows=(0, 99)), "n_rows"),
             (f(rows=(1, 17), n_thresholds=(0, 9)), "rows[1]"), (dict(f(rows=(1, 0), n_q=9), extra=None), "twice"),
             (dict(f(rows=(2, 16), n_thresholds=(0, 9)), extra=None), "extra"), (dict(f(n_thresholds=(1, 9)), nan_threshold=(0, 0)), "n_thresholds"),
             (dict(f(n_thresholds=(2, 2), n_q=9), nan_threshold=(2, 1)), "threshold[2][1]"), (f(n_q=9, q=(0, 2.0)), "n_q"),
             (dict(f(q=(1, 2.0)), factors=None), "q[1]"), ({"factors": None, "summary": None, "n": 0}, "factors"),
             ({"summary": None, "result": None}, "summary"), ({"result": None, "n": 0}, "result"), ({"n": 0, "ld": -1}, "n ="),
             ({"ld": 7, "ld_s": 7}, "ld ="), ({"ld_s": 7, "ctx": None}, "ld_s")]
    for kw, word in pairs:
        assert call_entry(lib, "ctx" not in kw, kw) == ERR_INVALID and word.encode() in lib.erpl_mc_last_error(), (kw, lib.erpl_mc_last_error())


# ------------------------------------------------------------------------------------------------ law_change
def test_law_change_of_the_default_table():
    K = 100
    target = {"mass_uncertainty": 0.01, "wind_speed_range": [3.0, 5.0], "initial_velocity": [0.05, 0.2, 0.1],
              "initial_attitude": [0.0025, 0.005, 0.01], "wind_direction_range": [math.pi / 2, math.pi]}
    motor, tm = models.LiquidMotor(), models.LiquidMotor()
    tm.thrust_uncertainty, tm.mass_flow_uncertainty = motor.thrust_uncertainty / 2, motor.mass_flow_uncertainty * 0.8
    got = sampling.law_change(K, True, None, target, motor=motor, target_motor=tm, shift={"motor_thrust": 0.5, "mass": -0.25})
    assert list(got) == [3, 4, 6, 8, 12, 14, 15, 317, 318]
    assert got[3] == (N, 0.0, 0.5, 0.0, 1.0) and got[4] == (N, 0.0, 2.0, 0.0, 1.0) and got[6] == (N, 0.0, 0.5, 0.0, 1.0)
    assert got[8] == (N, 0.0, 2.0, 0.0, 1.0) and got[12] == (N, -0.25, 0.5, 0.0, 1.0) and got[14] == (N, 0.5, 0.5, 0.0, 1.0)
    assert got[15][0] == N and math.isclose(got[15][2], 0.8) and got[317] == (U, 0.0, 1.0, 0.6, 1.0) and got[318] == (U, 0.0, 1.0, 0.25, 0.5)
    planar = sampling.law_change(K, True, None, target, motor=motor, target_motor=tm, planar=True)
    assert list(planar) == [3, 12, 14, 15, 317, 318]                       # velocity y, roll and yaw reach nothing in Set P
    assert sampling.law_change(K, True, None, {"mass_uncertainty": 0.02}) == {} and sampling.law_change(K, True, None, None, motor=motor) == {}
    assert list(sampling.law_change(K, False, None, None, motor=models.SolidMotor(), shift={"motor_thrust": 1.0, 20: 0.1})) == [14, 20]
    flown = {"mass_uncertainty": 0.04}
    assert sampling.law_change(K, True, flown, {"mass_uncertainty": 0.01})[12] == (N, 0.0, 0.25, 0.0, 1.0)


@pytest.mark.parametrize("kw,word", [
    ({"target": {"initial_position": [0.1, 0.0, 0.0]}}, "flown sigma is 0"),
    ({"target": {"mass_uncertainty": 0.0}}, "target sigma is 0"),
    ({"target": {"wind_speed_range": [0.0, 6.0]}}, "inside"), ({"target": {"wind_speed_range": [-1.0, 3.0]}}, "inside"),
    ({"target": {"wind_direction_range": [1.0, 1.0]}}, "inside"),
    ({"target": {"thrust_uncertainty": 0.01}}, "no primitive"), ({"target": {"atmospheric_density_uncertainty": 0.01}}, "no primitive"),
    ({"target": {"gravity": 1.0}}, "no entry"), ({"shift": {"wind_speed": 0.5}}, "shift"), ({"shift": {"dead_draw": 0.5}}, "shift"),
    ({"shift": {13: 0.5}}, "shift"), ({"shift": {"position_x": 0.5}}, "flown sigma"),
    ({"shift": {r: 0.1 for r in range(17, 17 + 33)}}, "more than"), ({"target_motor": models.LiquidMotor()}, "motor")])
def test_law_change_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        sampling.law_change(100, True, None, kw.get("target"), shift=kw.get("shift"), target_motor=kw.get("target_motor"))
