"""The ulp helper of tests/helpers.py and the committed input sets of tests/test_gpu_math.py, checked on the CPU."""
import numpy as np
import pytest

import helpers as H
import math_inputs as MI


def test_ulp_helper_spacing():
    f32, f64 = np.float32, np.float64
    # powers of two: the spacing above 2^k is that of [2^k, 2^(k+1)), the one just below it half of that
    for k in (-1000, -52, -1, 0, 1, 10, 52, 53, 1000):
        v = np.ldexp(1.0, k)
        assert H.ulp(v, f64) == np.nextafter(v, np.inf) - v == np.ldexp(1.0, k - 52)
        assert H.ulp(np.nextafter(v, 0.0), f64) == np.ldexp(1.0, k - 53)
    for k in (-100, -23, 0, 1, 24, 100):
        v = f32(np.ldexp(1.0, k))
        assert H.ulp(v, f32) == float(np.nextafter(v, f32(np.inf))) - float(v) == np.ldexp(1.0, k - 23)
        assert H.ulp(np.nextafter(v, f32(0)), f32) == np.ldexp(1.0, k - 24)
    assert H.ulp(-3.0, f64) == H.ulp(3.0, f64) == np.ldexp(1.0, -51)
    # the denormal boundary: the smallest normal number and everything below it, 0 included, is spaced by the smallest denormal
    for dt in (f32, f64):
        fi = np.finfo(dt)
        den = float(np.nextafter(dt(0), dt(1)))
        tiny = float(fi.tiny)
        assert H.ulp(tiny, dt) == den and H.ulp(tiny / 2, dt) == den and H.ulp(den, dt) == den and H.ulp(0.0, dt) == den
        assert H.ulp(2 * tiny, dt) == 2 * den
        assert H.ulp(float(fi.max), dt) == float(fi.max) - float(np.nextafter(fi.max, dt(0)))
    # fp32 against fp64 spacing: 2^29 apart at every normal fp32 value
    v = np.array([1.0, 1.5, 2.0, 3.14159, 1e-30, 1e30, 2.5e4])
    assert np.array_equal(H.ulp(v, f32), H.ulp(v, f64) * 2.0 ** 29)
    assert 2.3e-7 < H.ulp(2.5, f32) < 2.4e-7          # the fp32 angles past 2 rad are 2.4e-7 rad apart
    # vectorised, and the error itself: one ulp off is 1.0, the reference's tail counts
    assert np.array_equal(H.ulp_error([1.0 + 2.0 ** -52, 2.0], np.array([1.0, 2.0]), np.zeros(2), f64), [1.0, 0.0])
    assert H.ulp_error([1.0], np.array([1.0]), np.array([2.0 ** -54]), f64)[0] == 0.25
    assert np.isinf(H.ulp_error([np.nan, np.inf], np.ones(2), np.zeros(2), f64)).all()


def test_reference_split_is_exact_to_double_double():
    import mpmath
    x = np.array([0.1, 1.044, 3.0, 1e-300])
    hi, lo = MI.reference("log2", x, np.ones(4))
    with mpmath.workprec(MI.PREC_BITS):
        for a, h, l in zip(x, hi, lo):
            r = mpmath.log(mpmath.mpf(float(a))) / mpmath.log(2)
            assert abs(mpmath.mpf(float(h)) + mpmath.mpf(float(l)) - r) <= abs(r) * mpmath.mpf(2) ** -100
            assert abs(l) <= H.ulp(h, np.float64) / 2


ASSERTED = (("rcp", "rcp"), ("rsq", "rsq"), ("sqrt", "sqrt"), ("exp2", "exp2"), ("log2", "log2"), ("exp", "exp"),
            ("pow", "pow"), ("div", "div"), ("atan2", "angles"), ("atan2_abs", "angles"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_input_sets_have_finite_references(dtype):
    """Where test_gpu_math.py asserts a bound, the input is a value of the working precision and the reference is
    finite in it; where the bound is a hardware instruction's '1 ulp on normal operands', operands and results are
    normal numbers of the format as well (fp32: no denormal enters or leaves v_rcp / v_rsq / v_sqrt / v_exp / v_log)."""
    fi = np.finfo(dtype)
    for fn, name in ASSERTED:
        x, y = MI.inputs(name, dtype)
        assert x.shape == y.shape and x.size >= 20000, name
        assert np.array_equal(MI.cast(x, dtype), x) and np.array_equal(MI.cast(y, dtype), y), name
        assert np.isfinite(x).all() and np.isfinite(y).all(), name
        hi, lo = MI.reference_of(fn, name, dtype)
        assert np.isfinite(hi).all() and np.isfinite(lo).all(), (fn, name)
        assert np.abs(hi).max() <= float(fi.max), (fn, name)
        if name == "exp2" and dtype == np.float64:
            assert (hi[x >= -1074] > 0).all() and hi.min() >= 0        # denormal results are part of this set
            continue
        nz = hi != 0                                                     # exact zeros: log2(1), atan2(+-0, x > 0)
        assert np.abs(hi[nz]).min() >= float(fi.tiny) and (nz.all() or name in ("angles", "log2")), (fn, name)
        assert np.abs(x[x != 0]).min() >= float(fi.tiny) and ((x != 0).all() or name in ("angles", "exp2")), name
    # the sets hold what they are there for
    x, _ = MI.inputs("exp2", dtype)
    assert (x == np.floor(x)).sum() >= 150 and (x - np.floor(x) == 0.5).sum() >= 150
    x, _ = MI.inputs("log2", dtype)
    for k in (-1, 0, 1, 2):
        s = dtype(np.sqrt(0.5) * 2.0 ** k)
        assert (x == float(s)).any() and (x == float(np.nextafter(s, dtype(0)))).any() and (x == float(np.nextafter(s, dtype(9)))).any()
    x, y = MI.inputs("angles", dtype)
    assert ((x < 0) & (y == 0) & np.signbit(y)).any() and ((x < 0) & (y == 0) & ~np.signbit(y)).any() and ((x == 0) & (y != 0)).any()
    t = np.abs(np.arctan2(y, np.abs(x)))
    assert ((t > np.pi / 4 - 1e-6) & (t < np.pi / 4)).sum() >= 100 and ((t > np.pi / 4) & (t < np.pi / 4 + 1e-6)).sum() >= 100
