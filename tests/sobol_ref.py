"""The tests' own pick-freeze estimators (NumPy) and the rounding-error bounds a recursive summation of them may reach.

Y is [k + 2, m]: row 0 block A, row 1 block B, row 2 + i block AB_i (A with factor i taken from B), over the population.
  f0   = (sum yA + sum yB) / (2 m)
  V    = (sum (yA - f0)^2 + sum (yB - f0)^2) / (2 m)
  S1_i = (sum (yB - f0) d_i / m) / V           d_i = yAB_i - yA          (Saltelli et al. 2010, centred)
  ST_i = (sum d_i d_i / (2 m)) / V                                        (Jansen 1999)
V == 0 gives NaN indices.

The bounds (u = 2^-53; any order of summing n terms x is within n u sum|x| of the exact sum, Higham 2002 section 4.2; every
other operation is within u of its exact result):
  e0  = (2 m + 2) u mean|y|                                  f0: 2 m terms, one division
  c   = y - f0 as computed is within e0 + u |c| of the exact c, so c^2 within 2 |c| e0 + 2 e0^2 + 3 u c^2 (with its own
        rounding, second order in u dropped into the constants)
  bV  = (2 e0 sum|c| + 2 (2 m) e0^2 + (2 m + 5) u sum c^2) / (2 m)
  bN  = (e0 sum|d| + (m + 4) u sum|cB d|) / m + u |N|        N = sum (yB - f0) d / m
  bT  = (m + 3) u sum d^2 / (2 m) + u T                      T = sum d^2 / (2 m)
  a quotient x / V with x within bx and V within bV < V: within (bx + |x / V| bV) / (V - bV) + 2 u |x / V|."""
import numpy as np

U = 2.0 ** -53


def estimate(Y, dtype=np.float64):
    """(f0, V, S1 [k], ST [k]) of Y [k + 2, m] in `dtype` arithmetic."""
    Y = np.asarray(Y).astype(dtype)
    k, m = Y.shape[0] - 2, Y.shape[1]
    ya, yb = Y[0], Y[1]
    two_m = dtype(2 * m)
    f0 = (ya.sum(dtype=dtype) + yb.sum(dtype=dtype)) / two_m
    ca, cb = ya - f0, yb - f0
    V = ((ca * ca).sum(dtype=dtype) + (cb * cb).sum(dtype=dtype)) / two_m
    d = Y[2:] - ya
    with np.errstate(invalid="ignore", divide="ignore"):
        if V == 0:
            S1 = ST = np.full(k, np.nan, dtype=dtype)
        else:
            S1 = ((cb * d).sum(axis=1, dtype=dtype) / dtype(m)) / V
            ST = ((d * d).sum(axis=1, dtype=dtype) / two_m) / V
    return f0, V, S1, ST


def bounds(Y):
    """(exact f0, V, S1, ST as float64 of a long double evaluation, and the bounds e0, bV, bS1 [k], bST [k])."""
    L = np.longdouble
    f0, V, S1, ST = estimate(Y, L)
    Y = np.asarray(Y).astype(L)
    k, m = Y.shape[0] - 2, Y.shape[1]
    ya, yb = Y[0], Y[1]
    u = L(U)
    e0 = (2 * m + 2) * u * (np.abs(ya).sum() + np.abs(yb).sum()) / (2 * m)
    ca, cb = ya - f0, yb - f0
    abs_c, sq_c = np.abs(ca).sum() + np.abs(cb).sum(), (ca * ca).sum() + (cb * cb).sum()
    bV = (2 * e0 * abs_c + 2 * (2 * m) * e0 * e0 + (2 * m + 5) * u * sq_c) / (2 * m)
    d = Y[2:] - ya
    N = (cb * d).sum(axis=1) / m
    T = (d * d).sum(axis=1) / (2 * m)
    bN = (e0 * np.abs(d).sum(axis=1) + (m + 4) * u * np.abs(cb * d).sum(axis=1)) / m + u * np.abs(N)
    bT = (m + 3) * u * (d * d).sum(axis=1) / (2 * m) + u * T
    with np.errstate(invalid="ignore", divide="ignore"):
        bS1 = (bN + np.abs(S1) * bV) / (V - bV) + 2 * u * np.abs(S1)
        bST = (bT + np.abs(ST) * bV) / (V - bV) + 2 * u * np.abs(ST)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    return (f64(f0), f64(V), f64(S1), f64(ST)), (f64(e0), f64(bV), f64(bS1), f64(bST)), bool(bV < V / 2)


def check(got, Y, what=""):
    """got = (f0, V, S1 [k], ST [k]) of the code under test against the bounds of Y; returns the worst share of a bound."""
    (f0, V, S1, ST), (e0, bV, bS1, bST), solid = bounds(Y)
    assert solid, (what, "the data leave no variance to bound the indices with")
    worst = 0.0
    for name, g, want, bound in (("f0", got[0], f0, e0), ("V", got[1], V, bV), ("S1", got[2], S1, bS1), ("ST", got[3], ST, bST)):
        g, want, bound = np.atleast_1d(g), np.atleast_1d(want), np.atleast_1d(bound)
        err = np.abs(g - want)
        assert np.all(err <= bound), (what, name, g, want, bound)
        share = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
        worst = max(worst, float(share.max()))
    return worst


def ishigami(x, a=7.0, b=0.1):
    """x [3, n] on [-pi, pi]."""
    return np.sin(x[0]) + a * np.sin(x[1]) ** 2 + b * x[2] ** 4 * np.sin(x[0])


ISHIGAMI_S1 = (0.3139, 0.4424, 0.0)
ISHIGAMI_ST = (0.5576, 0.4424, 0.2437)


def ishigami_design(n_base=16384, seed=2024):
    """Y [5, n_base] of the pick-freeze design of the CPU test: A and B uniform on [-pi, pi] from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-np.pi, np.pi, (3, n_base))
    B = rng.uniform(-np.pi, np.pi, (3, n_base))
    rows = [ishigami(A), ishigami(B)]
    for i in range(3):
        AB = A.copy()
        AB[i] = B[i]
        rows.append(ishigami(AB))
    return np.vstack(rows)
