"""The tests' own restatement of the contract of erpl_mc_surrogate (include/erpl_mc.h) in NumPy: tables, recurrences, the
enumeration of the terms, the value of a term and of the polynomial operation for operation (so that predictions compare
bit for bit), the listwise population with its holdout, the least-squares fit and what is derived from coefficients."""
import itertools
import math

import numpy as np

UNIFORM, NORMAL = 0, 1
MAX_DEGREE = 12


def tables():
    k = np.arange(MAX_DEGREE + 1, dtype=np.float64)
    fact = np.array([float(math.factorial(i)) for i in range(MAX_DEGREE + 1)])
    return {"a": (2.0 * k + 1.0) / (k + 1.0), "b": k / (k + 1.0), "s": np.sqrt(2.0 * k + 1.0), "h": 1.0 / np.sqrt(fact)}


def count(n_vars, degree, order):
    return 1 + sum(math.comb(n_vars, o) * math.comb(g - 1, o - 1)
                   for g in range(1, degree + 1) for o in range(1, min(order, g, n_vars) + 1))


def _compositions(g, o):
    """The tuples of o integers >= 1 that sum to g, in lexicographic order."""
    if o == 1:
        yield (g,)
        return
    for first in range(1, g - o + 2):
        for rest in _compositions(g - first, o - 1):
            yield (first,) + rest


def terms(n_vars, degree, order):
    """int8 [P, 4, 2]: (variable, degree) of every factor of every term, unused slots (-1, 0)."""
    out = [[(-1, 0)] * 4]
    for g in range(1, degree + 1):
        for o in range(1, min(order, g, n_vars) + 1):
            for var in itertools.combinations(range(n_vars), o):
                for deg in _compositions(g, o):
                    out.append(list(zip(var, deg)) + [(-1, 0)] * (4 - o))
    return np.array(out, dtype=np.int8).reshape(len(out), 4, 2)


def univariate(kinds, X, degree):
    """psi[v][k] for k = 0..degree: float64 [V, degree + 1, n], by the contract's recurrences."""
    t = tables()
    X = np.asarray(X, dtype=np.float64)
    V, n = X.shape
    psi = np.empty((V, degree + 1, n))
    with np.errstate(all="ignore"):
        for v in range(V):
            psi[v, 0] = 1.0
            if kinds[v] == NORMAL:
                z = X[v]
                prev, cur = np.ones(n), z.copy()
                psi[v, 1] = t["h"][1] * cur
                for k in range(1, degree):
                    prev, cur = cur, (z * cur) - (float(k) * prev)
                    psi[v, k + 1] = t["h"][k + 1] * cur
            else:
                x = 2.0 * X[v] - 1.0
                prev, cur = np.ones(n), x.copy()
                psi[v, 1] = t["s"][1] * cur
                for k in range(1, degree):
                    prev, cur = cur, ((t["a"][k] * x) * cur) - (t["b"][k] * prev)
                    psi[v, k + 1] = t["s"][k + 1] * cur
    return psi


def basis(kinds, X, tm, degree):
    """Psi [P, n]: every term as the product of its factors in ascending variable order, starting from the first one."""
    psi = univariate(kinds, X, degree)
    n = psi.shape[2]
    out = np.empty((len(tm), n))
    with np.errstate(all="ignore"):
        for t, term in enumerate(tm):
            if term[0, 0] < 0:
                out[t] = 1.0
                continue
            v = psi[term[0, 0], term[0, 1]].copy()
            for s in range(1, 4):
                if term[s, 0] < 0:
                    break
                v = v * psi[term[s, 0], term[s, 1]]
            out[t] = v
    return out


def predict(kinds, degree, tm, coef, X):
    """[R, n]: acc = c_0, then acc = acc + (c_t Psi_t) in ascending term index; NaN where an input is not finite."""
    X = np.asarray(X, dtype=np.float64)
    Psi = basis(kinds, X, tm, degree)
    coef = np.atleast_2d(coef)
    out = np.empty((coef.shape[0], X.shape[1]))
    bad = ~np.all(np.isfinite(X), axis=0)
    with np.errstate(all="ignore"):
        for j, c in enumerate(coef):
            acc = np.full(X.shape[1], c[0])
            for t in range(1, len(tm)):
                acc = acc + (c[t] * Psi[t])
            out[j] = acc
    out[:, bad] = np.nan
    return out


def population(factors, ys, mask, holdout):
    """(members, fitted, held out) as sample indices, ascending, and (n_masked, n_non_finite)."""
    n = factors.shape[1]
    masked = np.zeros(n, dtype=bool) if mask is None else np.asarray(mask) != 0
    finite = np.all(np.isfinite(factors), axis=0) & np.all(np.isfinite(ys), axis=0)
    members = np.flatnonzero(~masked & finite)
    d = np.arange(len(members))
    held = (d % holdout == holdout - 1) if holdout else np.zeros(len(members), dtype=bool)
    return members, members[~held], members[held], int(masked.sum()), int((~masked & ~finite).sum())


def derived(coef, tm, n_vars):
    """mean, variance_pce, first [V], total [V], pair [V, V] of one row of coefficients."""
    c = np.asarray(coef, dtype=np.float64)
    sq = c * c
    var = 0.0
    first, total, pair = np.zeros(n_vars), np.zeros(n_vars), np.zeros((n_vars, n_vars))
    for t in range(1, len(tm)):
        var += sq[t]
        used = [int(v) for v in tm[t, :, 0] if v >= 0]
        for v in used:
            total[v] += sq[t]
        if len(used) == 1:
            first[used[0]] += sq[t]
        if len(used) == 2:
            pair[used[0], used[1]] += sq[t]
            pair[used[1], used[0]] += sq[t]
    if var == 0.0:
        return c[0], var, np.full(n_vars, np.nan), np.full(n_vars, np.nan), np.full((n_vars, n_vars), np.nan)
    with np.errstate(invalid="ignore"):
        return c[0], var, first / var, total / var, pair / var


def residuals(y, yhat):
    """tss around the mean of y, rss and 1 - rss / tss (NaN for a zero tss or no member)."""
    if len(y) == 0:
        return np.nan, np.nan, np.nan
    tss = float(np.sum((y - np.mean(y)) ** 2))
    with np.errstate(invalid="ignore"):
        rss = float(np.sum((y - yhat) ** 2))
        return tss, rss, (np.nan if tss == 0.0 else 1.0 - rss / tss)


def fit(kinds, X, Y, degree, order):
    """Least squares of the basis at the columns of X to the rows of Y: (terms, coefficients [R, P], Psi, cond(G))."""
    tm = terms(len(kinds), degree, order)
    Psi = basis(kinds, X, tm, degree)
    G = Psi @ Psi.T
    coef = np.linalg.solve(G, Psi @ np.atleast_2d(Y).T).T
    return tm, coef, Psi, float(np.linalg.cond(G))


def ishigami(x1, x2, x3, a=7.0, b=0.1):
    return np.sin(x1) + a * np.sin(x2) ** 2 + b * x3 ** 4 * np.sin(x1)


def ishigami_analytic(a=7.0, b=0.1):
    """mean, variance, first [3], total [3], pair {(0, 2)} of Ishigami's function on (-pi, pi)^3."""
    pi = math.pi
    v1 = 0.5 * (1.0 + b * pi ** 4 / 5.0) ** 2
    v2 = a * a / 8.0
    v13 = b * b * pi ** 8 * (1.0 / 18.0 - 1.0 / 50.0)
    var = v1 + v2 + v13
    return a / 2.0, var, np.array([v1, v2, 0.0]) / var, np.array([v1 + v13, v2, v13]) / var, v13 / var
