"""The kernels' own arithmetic ON THE DEVICE: every m_* function of erpl_k_math.h, of all three builds, evaluated through
erpl_mc_debug_eval(ERPL_DBG_MATH) - the very functions, the constant-memory coefficient tables and the `early` operand of
the flight kernel - against mpmath at 240 bits.  The reference is taken at the input as the build sees it (fp32:
np.float32(x)); errors are in ulps of the working precision at the reference value (helpers.ulp_error; below the smallest
normal number that is the denormal spacing).  The input sets are in tests/math_inputs.py (fixed seeds, 20 000 - 32 000
points per function) and come from how the RHS uses each function.

What is asserted:
  * a bound the code documents and that holds is the assertion: m_rcp 1.0 ulp, m_rsq 1.24 ulp, m_exp2 2 ulp (fp64
    throughput build); the fp32 build's hardware instructions 1 ulp (v_rcp / v_rsq / v_sqrt / v_exp / v_log_f32);
  * a composition takes the first-order bound derived in its test's docstring from its primitives' bounds;
  * the gate build's (and the fp64 throughput build's library) sqrt and division are correctly rounded: equal to NumPy's;
    exp / pow / atan2 of the device library are printed; in the gate build, whose equality with the CPU oracle rests on
    them, they are held to the ulp limits of the OpenCL C specification (exp 3, pow 16, atan2 6), which that library
    implements.  The fp64 throughput build compiles the same library calls with FMA contraction on (its rail kernel's
    analytic atmosphere uses them): printed only - its pow measures 23 ulp, 2.6e-15 relative, against that build's
    5e-13 on the atmosphere;
  * m_log2 and the aerodynamic angles of the fp64 throughput build, and the fp32 angles, whose earlier comments ("<= 2 ulp",
    "1.0e-7 rad", "2e-7 rad") did not hold as written: the bound has the true form given in erpl_k_math.h and the number
    is 1.5 x the worst error MEASURED on the MI355X over the committed input set (the margin covers a compiler that
    contracts or schedules differently); for the fp64 functions it may not exceed 4 ulp of the result.
Each test prints its worst error and the input it occurred at; DESIGN.md section 5 holds the table."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, flatten, models

import helpers as H
import math_inputs as MI

pytestmark = pytest.mark.gpu

PRECISIONS = ["f64", "f64_fast", "f32"]
ROW = {"rcp": 0, "rsq": 1, "sqrt_pos": 2, "exp2": 3, "log2": 4, "exp": 5, "pow": 6, "div": 7, "atan2": 8, "clamp": 9,
       "alpha": 10, "beta": 11, "alpha_single": 12, "beta_single": 13, "next_up": 14, "sqrt": 15}
# rows a build has no function for: NaN
MISSING = {"f64": ("rsq", "exp2", "log2", "clamp", "alpha", "beta", "alpha_single", "beta_single"),
           "f64_fast": (), "f32": ("alpha_single", "beta_single")}

# Worst errors measured on the MI355X over the committed input sets (see the table in DESIGN.md); asserted x 1.5.
MEASURED = {
    "f64_fast log2, ulps at max(|log2 x|, 1)": 0.982,          # x = 2.7132940126463496 (3.040 ulp of the result at 1.4142135620073792)
    "f64_fast alpha, ulps of the result": 3.017,               # x = 5.659713781013323e-05, y = 5.659713793809075e-05 (the fold)
    "f64_fast beta, ulps of the result": 3.017,                # the same point
    "f32 atan2, ulps of the result beyond 4.5e-8 rad": 1.861,  # x = 8.664160e-06, y = 8.880444e-06 (0.798 rad)
    "f32 alpha, ulps of the result beyond 9e-8 rad": 2.330,    # x = -0.5587607, y = -26.93943 (-1.59 rad: 3.7e-7 rad in all)
    "f32 beta, ulps of the result beyond 9e-8 rad": 1.860,     # x = 7137.976, y = -292481.97 (-1.546 rad)
}
MARGIN = 1.5
FP64_CEILING = 4.0     # ulps of the result: 3 from an exact-FMA emulation of the code + the 1 ulp m_rcp may add


def asserted(key, ceiling=np.inf):
    """1.5 x the measured worst; for the fp64 functions never more than the ceiling the code's structure allows."""
    return min(MARGIN * MEASURED[key], ceiling)


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def evaluate(engine):
    """evaluate(precision, x, y) -> the [ERPL_DBG_MATH_ROWS, m] table of the build; evaluate.on(precision, name) the same
    over a committed input set, computed once."""
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    hb = flatten.HostBatch(1, 0)
    r = models.Rocket()
    hb.rocket[:, 0] = [r.dry_mass, r.propellant_mass]
    hb.motor[:, 0] = flatten.motor_row(H.make_motor("liquid"))
    hb.ic[6, 0] = 1.0
    dbs = {p: DeviceBatch.from_host(hb, engine.device, _abi.PRECISIONS[p]) for p in PRECISIONS}
    cache = {}

    def run(precision, x, y=None):
        x = np.asarray(x, dtype=np.float64)
        y = np.ones_like(x) if y is None else np.asarray(y, dtype=np.float64)
        out = engine.debug_eval(dbs[precision], _abi.DBG_MATH, np.stack([x, y]))
        assert out.shape == (_abi.DBG_MATH_ROWS, x.size)
        return out

    def on(precision, name):
        if (precision, name) not in cache:
            cache[precision, name] = run(precision, *MI.inputs(name, MI.DTYPES[precision]))
        return cache[precision, name]
    run.on = on
    return run


def worst(label, err, x, y=None):
    """Print the worst error and where it occurred; return it."""
    j = int(np.argmax(err))
    at = f"x = {x[j]!r}" + ("" if y is None else f", y = {y[j]!r}")
    print(f"{label}: worst {err[j]:.3f} at {at} over {err.size} points")
    return float(err[j])


def ulp_err(precision, got, fn, name):
    return H.ulp_error(got, *MI.reference_of(fn, name, MI.DTYPES[precision]), MI.DTYPES[precision])


def klass(v):
    """nan / +inf / -inf / +0 / -0 / finite of every value."""
    v = np.asarray(v, dtype=np.float64)
    sign = np.where(np.signbit(v), "-", "+")
    return [("nan" if np.isnan(a) else s + "inf" if np.isinf(a) else s + "0" if a == 0 else "finite") for a, s in zip(v, sign)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_missing_rows_are_nan(evaluate, precision):
    out = evaluate(precision, [0.5, 2.0, 3.0], [0.25, 1.5, -2.0])
    for name, row in ROW.items():
        assert np.isnan(out[row]).all() == (name in MISSING[precision]), name


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rcp(evaluate, precision):
    """fp64 throughput build: v_rcp_f64 seed + one cubic round, documented within 1.0 ulp; fp32: v_rcp_f32, 1 ulp; the gate's
    1.0 / a is IEEE division."""
    x, _ = MI.inputs("rcp", MI.DTYPES[precision])
    got = evaluate.on(precision, "rcp")[ROW["rcp"]]
    e = worst(f"{precision} m_rcp [ulp]", ulp_err(precision, got, "rcp", "rcp"), x)
    if precision == "f64":
        assert np.array_equal(got, 1.0 / x)
    assert e <= (0.5 if precision == "f64" else 1.0)


@pytest.mark.parametrize("precision", ["f64_fast", "f32"])
def test_rsq(evaluate, precision):
    """fp64 throughput build: v_rsq_f64 seed + one cubic round, documented 1.24 ulp; fp32: v_rsq_f32, 1 ulp.  (The gate
    build has no m_rsq: test_missing_rows_are_nan.)"""
    x, _ = MI.inputs("rsq", MI.DTYPES[precision])
    got = evaluate.on(precision, "rsq")[ROW["rsq"]]
    e = worst(f"{precision} m_rsq [ulp]", ulp_err(precision, got, "rsq", "rsq"), x)
    assert e <= (1.24 if precision == "f64_fast" else 1.0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sqrt(evaluate, precision):
    """m_sqrt of the fp64 builds is the library's correctly rounded sqrt (equal to NumPy's); the fp32 build's is v_sqrt_f32,
    1 ulp.  m_sqrt_pos of the fp64 throughput build is x m_rsq(x): with y = m_rsq(x) within 1.24 ulp(y) and the product
    rounded once, |error| <= 1.24 ulp(y) x + 0.5 ulp(r); ulp(y) / y and ulp(r) / r both lie in (2^-53, 2^-52], so
    ulp(y) x <= 2 ulp(r) (reached for x just below 4^k) and the bound is 2 * 1.24 + 0.5 = 2.98 ulp."""
    x, _ = MI.inputs("sqrt", MI.DTYPES[precision])
    out = evaluate.on(precision, "sqrt")
    if precision == "f32":
        assert np.array_equal(out[ROW["sqrt"]], out[ROW["sqrt_pos"]])
        e = worst("f32 m_sqrt [ulp]", ulp_err(precision, out[ROW["sqrt"]], "sqrt", "sqrt"), x)
        assert e <= 1.0
        return
    assert np.array_equal(out[ROW["sqrt"]], np.sqrt(x))
    e = worst(f"{precision} m_sqrt_pos [ulp]", ulp_err(precision, out[ROW["sqrt_pos"]], "sqrt", "sqrt"), x)
    if precision == "f64":
        assert np.array_equal(out[ROW["sqrt_pos"]], np.sqrt(x))
    else:
        assert e <= 2.98


# What 0, -0, +inf, -inf, NaN (and -1 for the roots) give: the IEEE value or NaN, never a finite number.  The cubic round of
# the fp64 throughput build turns m_rcp(0) and m_rcp(inf) into NaN (e = 1 - 0 * inf), likewise m_rsq; m_sqrt_pos(+inf) is
# NaN by the code's own comment.  Pinned, so that a rewrite cannot change them unnoticed.
SPECIAL_X = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0]
SPECIALS = {
    "f64": {"rcp": ["+inf", "-inf", "+0", "-0", "nan"], "sqrt_pos": ["+0", "-0", "+inf", "nan", "nan", "nan"]},
    "f64_fast": {"rcp": ["nan"] * 5, "rsq": ["nan"] * 6, "sqrt_pos": ["nan"] * 6},
    "f32": {"rcp": ["+inf", "-inf", "+0", "-0", "nan"], "rsq": ["+inf", "-inf", "+0", "nan", "nan", "nan"],
            "sqrt_pos": ["+0", "-0", "+inf", "nan", "nan", "nan"]},
}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rcp_rsq_sqrt_specials(evaluate, precision):
    out = evaluate(precision, SPECIAL_X)
    for name, exp in SPECIALS[precision].items():
        got = klass(out[ROW[name]][:len(exp)])
        print(f"{precision} m_{name} of {SPECIAL_X[:len(exp)]}: {got}")
        assert "finite" not in got and got == exp, name


@pytest.mark.parametrize("precision", ["f64_fast", "f32"])
def test_exp2(evaluate, precision):
    """fp64 throughput build: documented <= 2 ulp over [-1100, 30], in denormal spacing below -1022; integers are exact
    (f = 0, p = 1); x < -1100 and -inf give 0, 1024 gives inf, NaN gives NaN.  fp32: v_exp_f32, 1 ulp on normal results."""
    x, _ = MI.inputs("exp2", MI.DTYPES[precision])
    got = evaluate.on(precision, "exp2")[ROW["exp2"]]
    err = ulp_err(precision, got, "exp2", "exp2")
    e = worst(f"{precision} m_exp2 [ulp]", err, x)
    sp = evaluate(precision, [-np.inf, np.nan, 1024.0, -1101.0, -2000.0, -1e300, -1074.0, -1075.0])[ROW["exp2"]]
    assert sp[0] == 0 and np.isnan(sp[1]) and sp[2] == np.inf
    if precision == "f64_fast":
        assert e <= 2.0
        den = x < -1022
        print(f"f64_fast m_exp2: {den.sum()} points with denormal results, worst {err[den].max():.3f} denormal spacings")
        assert den.sum() >= 1000
        n = x == np.floor(x)
        assert np.array_equal(got[n], np.ldexp(1.0, x[n].astype(int)))
        assert np.array_equal(sp[3:6], [0.0, 0.0, 0.0]) and sp[6] == 2.0 ** -1074 and sp[7] in (0.0, 2.0 ** -1074)
    else:
        assert e <= 1.0


@pytest.mark.parametrize("precision", ["f64_fast", "f32"])
def test_log2(evaluate, precision):
    """fp64 throughput build: log2 x = e + s q(s^2) with s = (m - 1) m_rcp(m + 1).  The "<= 2 ulp" of the earlier comment
    does not hold in ulps of the result (an exact-FMA emulation finds 2.94 near x = 1.044); what holds is an absolute error
    relative to max(|log2 x|, 1).  Asserted: 1.5 x the measured worst in ulps at max(|log2 x|, 1), and the 4 ulp ceiling in
    ulps of the result.  Powers of two are exact (s == 0).  fp32: v_log_f32, 1 ulp of the result."""
    dtype = MI.DTYPES[precision]
    x, _ = MI.inputs("log2", dtype)
    got = evaluate.on(precision, "log2")[ROW["log2"]]
    hi, lo = MI.reference_of("log2", "log2", dtype)
    e_res = worst(f"{precision} m_log2 [ulp of the result]", H.ulp_error(got, hi, lo, dtype), x)
    p2 = MI.powers_of_two(dtype)
    gp = evaluate(precision, p2)[ROW["log2"]]
    if precision == "f64_fast":
        with np.errstate(invalid="ignore"):
            e_abs = np.abs((got - hi) - lo) / H.ulp(np.maximum(np.abs(hi), 1.0), dtype)
        e_abs = worst("f64_fast m_log2 [ulp at max(|log2 x|, 1)]", np.where(np.isnan(e_abs), np.inf, e_abs), x)
        assert np.array_equal(gp, np.log2(p2))
        assert e_res <= FP64_CEILING
        assert e_abs <= asserted("f64_fast log2, ulps at max(|log2 x|, 1)", FP64_CEILING)
    else:
        print(f"f32 m_log2 of the powers of two: worst |error| {np.abs(gp - np.log2(p2)).max():.3g}")
        assert e_res <= 1.0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_div(evaluate, precision):
    """fp64 builds: IEEE division, equal to NumPy's.  fp32: a * v_rcp_f32(b): the reciprocal within 1 ulp, i.e. a relative
    error <= 2^-23 = 2 ulp of the quotient at most (ulp(q) >= 2^-24 |q|), and the product rounded once: 2 + 0.5 = 2.5 ulp."""
    x, y = MI.inputs("div", MI.DTYPES[precision])
    got = evaluate.on(precision, "div")[ROW["div"]]
    e = worst(f"{precision} m_div [ulp]", ulp_err(precision, got, "div", "div"), x, y)
    if precision == "f32":
        assert e <= 2.5
    else:
        assert np.array_equal(got, x / y) and e <= 0.5


LOG2E_F32 = float(np.float32(1.44269504088896341))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exp(evaluate, precision):
    """fp32: v_exp_f32(t), t = fl(x c), c = fl32(log2 e) = log2 e (1 + dc), the product rounded once (dm <= 2^-24): t =
    x log2 e (1 + dc + dm) to first order, so 2^t = e^x (1 + ln 2 x log2 e (dc + dm)) = e^x (1 + x (dc + dm)): a relative error
    |x| (|dc| + 2^-24), at most |x| (|dc| 2^24 + 1) ulps of the result, plus the instruction's own 1 ulp.  The bound grows
    with |x|: 1 + |x| (|dc| 2^24 + 1) ulp.  fp64 builds: the device library's exp, printed; the gate's held to OpenCL's 3 ulp."""
    x, _ = MI.inputs("exp", MI.DTYPES[precision])
    got = evaluate.on(precision, "exp")[ROW["exp"]]
    err = ulp_err(precision, got, "exp", "exp")
    e = worst(f"{precision} m_exp [ulp]", err, x)
    if precision == "f32":
        dc = abs(LOG2E_F32 - 1.44269504088896341) / 1.44269504088896341
        bound = 1.0 + np.abs(x) * (dc * 2.0 ** 24 + 1.0)
        assert worst("f32 m_exp [error / (1 + |x| (dc 2^24 + 1)) ulp]", err / bound, x) <= 1.0
    elif precision == "f64":
        assert e <= 3.0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pow(evaluate, precision):
    """fp32: v_exp_f32(t), t = fl(y L), L = v_log_f32(x) = log2 x (1 + d1) with |d1| <= 2^-23 (1 ulp), the product rounded
    once (d2 <= 2^-24): 2^t = x^y (1 + ln 2 y log2 x (d1 + d2)) to first order, a relative error ln 2 |y log2 x| 3 2^-24, at
    most 3 ln 2 |y log2 x| ulps of the result, plus the instruction's own 1 ulp: 1 + 3 ln 2 |y log2 x| ulp.
    fp64 builds: the device library's pow, printed; the gate's held to OpenCL's 16 ulp."""
    x, y = MI.inputs("pow", MI.DTYPES[precision])
    got = evaluate.on(precision, "pow")[ROW["pow"]]
    err = ulp_err(precision, got, "pow", "pow")
    e = worst(f"{precision} m_pow [ulp]", err, x, y)
    if precision == "f32":
        bound = 1.0 + 3.0 * np.log(2.0) * np.abs(y * np.log2(x))
        assert worst("f32 m_pow [error / (1 + 3 ln 2 |y log2 x|) ulp]", err / bound, x, y) <= 1.0
    elif precision == "f64":
        assert e <= 16.0


def angle_excess(got, fn, dtype, floor_rad):
    """max(0, |error| - floor_rad) in ulps of the result: the form  |error| <= floor_rad + k ulp(result)."""
    hi, lo = MI.reference_of(fn, "angles", dtype)
    with np.errstate(invalid="ignore"):
        d = np.abs((got - hi) - lo)
    d = np.where(np.isnan(d), np.inf, d)
    return np.maximum(d - floor_rad, 0.0) / H.ulp(hi, dtype), d


@pytest.mark.parametrize("precision", PRECISIONS)
def test_atan2(evaluate, precision):
    """fp32: octant reduction + odd minimax polynomial on [0, 1].  The polynomial's own error is 4.44e-8 rad, and fp32 values
    past 2 rad are 2.4e-7 rad apart, so "max error 1.0e-7 rad" cannot hold; the true form is |error| <= 4.5e-8 rad +
    k ulp(result), k asserted at 1.5 x the measured worst.  NaN in, NaN out.  (0, 0) is outside its contract.
    fp64 builds: the device library's atan2, printed; the gate's held to OpenCL's 6 ulp."""
    dtype = MI.DTYPES[precision]
    x, y = MI.inputs("angles", dtype)
    keep = (x != 0) | (y != 0)
    got = evaluate.on(precision, "angles")[ROW["atan2"]]
    e = worst(f"{precision} m_atan2 [ulp]", ulp_err(precision, got, "atan2", "angles")[keep], x[keep], y[keep])
    assert np.array_equal(np.signbit(got[keep]), np.signbit(y[keep]))
    if precision == "f32":
        k, d = angle_excess(got, "atan2", dtype, 4.5e-8)
        worst("f32 m_atan2 [rad]", d[keep], x[keep], y[keep])
        k = worst("f32 m_atan2 [ulp of the result beyond 4.5e-8 rad]", k[keep], x[keep], y[keep])
        assert k <= asserted("f32 atan2, ulps of the result beyond 4.5e-8 rad")
        nn = evaluate(precision, [np.nan, 1.0, np.nan], [1.0, np.nan, np.nan])[ROW["atan2"]]
        assert np.isnan(nn).all()
    elif precision == "f64":
        assert e <= 6.0


@pytest.mark.parametrize("precision", ["f64_fast", "f32"])
def test_aero_angles(evaluate, precision):
    """alpha = atan2(y, x) and beta = atan2(y, |x|) as the fast RHS calls m_aero_angles: through the half angle, with the
    length r = v2 m_rsq(v2) of the RHS (its rounding is part of what is measured).  atan2(0, 0) = 0 (floored length).
    fp64 throughput build: the "<= 2 ulp" of the earlier comment does not hold (2.92 ulp by emulation just past the
    tan(pi/8) fold; 3.02 measured on it); asserted: 1.5 x the measured worst in ulps of the result, capped at the 4 ulp
    ceiling (which is what binds here); the pair and the single form agree bit for bit ("same arithmetic").  fp32: twice the m_atan2 polynomial, |error| <= 9e-8 rad +
    k ulp(result), k asserted at 1.5 x the measured worst."""
    dtype = MI.DTYPES[precision]
    x, y = MI.inputs("angles", dtype)
    out = evaluate.on(precision, "angles")
    zero = (x == 0) & (y == 0)
    for name, fn in (("alpha", "atan2"), ("beta", "atan2_abs")):
        got = out[ROW[name]]
        assert np.array_equal(np.signbit(got), np.signbit(y)), name
        assert (got[zero] == 0).all()
        e = worst(f"{precision} {name} [ulp of the result]", ulp_err(precision, got, fn, "angles"), x, y)
        if precision == "f64_fast":
            assert np.array_equal(got, out[ROW[name + "_single"]]), name
            assert e <= asserted(f"f64_fast {name}, ulps of the result", FP64_CEILING), name
        else:
            k, d = angle_excess(got, fn, dtype, 9e-8)
            worst(f"f32 {name} [rad]", d, x, y)
            k = worst(f"f32 {name} [ulp of the result beyond 9e-8 rad]", k, x, y)
            assert k <= asserted(f"f32 {name}, ulps of the result beyond 9e-8 rad"), name


@pytest.mark.parametrize("precision", ["f64_fast", "f32"])
def test_clamp(evaluate, precision):
    """m_clamp(x, -1, hi): inside, outside and on the bounds; a NaN x gives the lower bound in both builds."""
    dtype = MI.DTYPES[precision]
    his = MI.cast([0.2617993877991494, 1e30, 0.0, -1.0], dtype)
    xs = MI.cast([-np.inf, -1e31, -2.0, -1.0000001, -1.0, -0.9999999, -0.5, 0.0, 0.1, 0.2617993877991494, 0.2617994, 0.3, 1.0,
                  1e30, 1.0000001e30, 1e31, np.inf], dtype)
    xs = np.concatenate([xs, np.nextafter(his.astype(dtype), dtype(-np.inf)).astype(np.float64),
                         np.nextafter(his.astype(dtype), dtype(np.inf)).astype(np.float64)])
    X, Y = [a.ravel() for a in np.meshgrid(xs, his)]
    got = evaluate(precision, X, Y)[ROW["clamp"]]
    assert np.array_equal(got, np.clip(X, -1.0, Y))
    assert ((X < -1) & (got == -1)).any() and ((X > Y) & (got == Y)).any() and ((X == Y) | (X == -1)).any()
    nan = evaluate(precision, np.full(his.size, np.nan), his)[ROW["clamp"]]
    assert np.array_equal(nan, np.full(his.size, -1.0))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_next_up(evaluate, precision):
    """m_next_up(x): the smallest value above a positive finite x (the closed atmosphere layer bounds as half-open ranges)."""
    dtype = MI.DTYPES[precision]
    rs = np.random.RandomState(5)
    x = MI.cast(np.concatenate([[11000.0, 20000.0, 25000.0, 32000.0, 1.0, float(np.finfo(dtype).tiny)],
                                MI.around_powers_of_two(-100, 100, dtype), 10.0 ** rs.uniform(-30, 30, 2000)]), dtype)
    got = evaluate(precision, x)[ROW["next_up"]]
    assert np.array_equal(got, np.nextafter(x.astype(dtype), dtype(np.inf)).astype(np.float64))
