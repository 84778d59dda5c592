"""Input sets and mpmath references of tests/test_gpu_math.py (shared with the CPU-side check of them in
tests/test_math_helpers.py).  Every set is a pair (x, y) of float64 arrays that hold values of the working precision
exactly - for fp32 the reference is evaluated at np.float32(x), the input as that build sees it - built from fixed
seeds; the references are mpmath values at 240 bits, kept as a float64 head and tail (ref = hi + lo to ~2^-106), so
that the comparison itself is vectorised.  The sets come from how the RHS uses each function (erpl_k_rhs_fast.h)."""
import functools

import mpmath
import numpy as np

PREC_BITS = 240
DTYPES = {"f64": np.float64, "f64_fast": np.float64, "f32": np.float32}


def cast(v, dtype):
    """The values as a build of working precision `dtype` sees them, held in float64."""
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=np.float64).astype(dtype).astype(np.float64)


def around_powers_of_two(k_lo, k_hi, dtype):
    """2^k for k_lo <= k <= k_hi (every 4^k among them) with the value one ulp below and one ulp above each."""
    p = np.ldexp(dtype(1), np.arange(k_lo, k_hi + 1)).astype(dtype)
    return np.concatenate([np.nextafter(p, dtype(0)), p, np.nextafter(p, dtype(np.inf))]).astype(np.float64)


def _log_uniform(rs, lo_exp, hi_exp, n):
    return 10.0 ** rs.uniform(lo_exp, hi_exp, n)


def _walk(v, steps, dtype):
    """v and the `steps` values of `dtype` on either side of it."""
    out, a, b = [dtype(v)], dtype(v), dtype(v)
    for _ in range(steps):
        a, b = np.nextafter(a, dtype(-np.inf)), np.nextafter(b, dtype(np.inf))
        out += [a, b]
    return np.array(out, dtype=np.float64)


def angle_points(rs, dtype):
    """(x, y) of the angle sets: the full circle at radii 1e-6 .. 1e6, clusters at 0, +-pi/2 and +-pi (x < 0 and y
    tending to +-0 among them), both sides of the tan(pi/8) fold of the half-angle form (|angle| = pi/4, and 3 pi/4
    behind the x < 0 reflection), y = +-0 and x = 0."""
    th = [rs.uniform(-np.pi, np.pi, 20000)]
    for c in (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, np.pi / 4, -np.pi / 4, 3 * np.pi / 4, -3 * np.pi / 4):
        d = 10.0 ** rs.uniform(-12, -1, 600) * rs.choice([-1.0, 1.0], 600)
        th.append(c + d)
    th = np.concatenate(th)
    r = _log_uniform(rs, -6, 6, th.size)
    x, y = r * np.cos(th), r * np.sin(th)
    tiny = 1e-300 if dtype == np.float64 else 1e-30
    ex = np.array([1.0, 1.0, -1.0, -1.0, 0.0, 0.0, -3.0, -3.0, 2.5e5, -2.5e5, 1e-6, -1e-6])
    ey = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, tiny, -tiny, tiny, -tiny, 1e-6, 1e-6])
    return cast(np.concatenate([x, ex]), dtype), cast(np.concatenate([y, ey]), dtype)


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """The committed input set of function `name` for working precision `dtype`: (x, y)."""
    f64 = dtype == np.float64
    rs = np.random.RandomState({"rcp": 11, "rsq": 12, "sqrt": 13, "exp2": 14, "log2": 15, "exp": 16, "pow": 17,
                                "div": 18, "angles": 19}[name])
    y = None
    if name == "rcp":      # 1e-6 .. 1e12, both signs; one ulp either side of the powers of two
        m = _log_uniform(rs, -6, 12, 20000) * rs.choice([-1.0, 1.0], 20000)
        p = around_powers_of_two(-20, 40, dtype)
        x = np.concatenate([m, p, -p])
    elif name == "rsq":    # up to 1e24: squared speeds below the hand-over are 1e12; quaternion norms sit near 0.5
        x = np.concatenate([_log_uniform(rs, -6, 24, 20000), rs.uniform(0.4, 0.6, 2000), around_powers_of_two(-20, 80, dtype)])
    elif name == "sqrt":
        x = np.concatenate([_log_uniform(rs, -6, 12, 20000), around_powers_of_two(-20, 40, dtype)])
    elif name == "exp2":   # every integer (exact) and every tie n + 1/2 (rint goes to even), dense on [-1, 1]
        lo, n_lo = (-1100.0, -1080) if f64 else (-125.0, -125)
        n = np.arange(n_lo, 31, dtype=np.float64)
        x = np.concatenate([rs.uniform(lo, 30.0, 20000), rs.uniform(-1.0, 1.0, 10000), n, n[:-1] + 0.5] +
                           ([np.array([-1074.0, -1075.0])] if f64 else []))
    elif name == "log2":   # [1/4, 4], dense around 1 and either side of every sqrt(1/2) 2^k split; sparse over the range
        near1 = 1.0 + 10.0 ** rs.uniform(-16 if f64 else -7, -1, 4000) * rs.choice([-1.0, 1.0], 4000)
        parts = [rs.uniform(0.25, 4.0, 20000), near1, _walk(1.0, 16, dtype)]
        for k in (-1, 0, 1, 2):
            s = np.sqrt(0.5) * 2.0 ** k
            parts += [_walk(s, 16, dtype), s * (1.0 + 10.0 ** rs.uniform(-15 if f64 else -7, -2, 500) * rs.choice([-1.0, 1.0], 500))]
        e = 300 if f64 else 37
        parts.append(_log_uniform(rs, -e, e, 2000))
        x = np.concatenate(parts)
    elif name == "exp":    # results stay normal in the working precision
        x = np.concatenate([rs.uniform(*((-700.0, 700.0) if f64 else (-80.0, 20.0)), 20000), rs.uniform(-1.0, 1.0, 10000)])
    elif name == "pow":    # the atmosphere's (T / Tref)^e: bases around 1, exponents 5.26 and -34.2
        x = np.concatenate([rs.uniform(0.5, 1.5, 16000), 1.0 + 10.0 ** rs.uniform(-7, -1, 4000) * rs.choice([-1.0, 1.0], 4000)])
        y = np.concatenate([rs.uniform(-40.0, 10.0, 18000), np.full(1000, 5.255877), np.full(1000, -34.1632)])
    elif name == "div":
        x = _log_uniform(rs, -6, 8, 20000) * rs.choice([-1.0, 1.0], 20000)
        y = _log_uniform(rs, -6, 8, 20000) * rs.choice([-1.0, 1.0], 20000)
    elif name == "angles":
        return angle_points(rs, dtype)
    else:
        raise KeyError(name)
    x = cast(x, dtype)
    y = np.ones_like(x) if y is None else cast(y, dtype)
    return x, y


def powers_of_two(dtype):
    """Every normal power of two of `dtype`."""
    fi = np.finfo(dtype)
    return np.ldexp(1.0, np.arange(fi.minexp, fi.maxexp))


_MP = {
    "rcp": lambda x, y: 1 / x,
    "rsq": lambda x, y: 1 / mpmath.sqrt(x),
    "sqrt": lambda x, y: mpmath.sqrt(x),
    "exp2": lambda x, y: mpmath.power(2, x),
    "log2": lambda x, y: mpmath.log(x) / mpmath.log(2),
    "exp": lambda x, y: mpmath.exp(x),
    "pow": lambda x, y: mpmath.power(x, y),
    "div": lambda x, y: x / y,
    "atan2": lambda x, y: mpmath.atan2(y, x),             # alpha: any x
    "atan2_abs": lambda x, y: mpmath.atan2(y, abs(x)),    # beta: x >= 0
}


def reference(fn, x, y):
    """mpmath value of `fn` at every (x, y) as (hi, lo) float64 arrays, ref = hi + lo."""
    with mpmath.workprec(PREC_BITS):
        f = _MP[fn]
        r = [f(mpmath.mpf(float(a)), mpmath.mpf(float(b))) for a, b in zip(x, y)]
        if fn.startswith("atan2"):   # mpmath has no signed zero: atan2(-0, x) = -atan2(+0, x), i.e. -pi for x < 0
            r = [-v if (b == 0 and np.signbit(b)) else v for v, b in zip(r, y)]
        hi = np.array([float(v) for v in r])
        lo = np.array([float(v - mpmath.mpf(h)) for v, h in zip(r, hi)])
    return hi, lo


@functools.lru_cache(maxsize=None)
def reference_of(fn, name, dtype):
    """Reference of `fn` over the committed input set `name` (computed once per session)."""
    x, y = inputs(name, dtype)
    return reference(fn, x, y)
