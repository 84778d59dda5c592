"""erpl_mc_corridor_drivers restated in NumPy from the definitions in include/erpl_mc.h: populations, two-pass moments, Pearson
over every row's own population and the standardised regression by Cholesky with the pivot rule of erpl_mc_correlation.  No
standardised sums, no slices: the plain two-pass formulae, row by row.  tests/test_corridor_drivers_ref.py holds it to
np.corrcoef and np.linalg.lstsq; tests/test_gpu_corridor_drivers.py holds the device to it.  Also the generator of the data
both use."""
import numpy as np

NAN = float("nan")
PIVOT = 1e-10


def _cholesky(R):
    """(L or None, smallest pivot met - the failing one included; NaN for an empty matrix): the rule of erpl_mc_correlation."""
    k = R.shape[0]
    L = np.zeros((k, k))
    low = NAN
    for i in range(k):
        for j in range(i + 1):
            s = R[i, j] - np.dot(L[i, :j], L[j, :j])
            if i == j:
                if not (low <= s):
                    low = s
                if not (s >= PIVOT) or not np.isfinite(s):
                    return None, low
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return L, low


def restate(factors, values, mask=None, m=None, regression=True):
    """factors [F, ldf], values [R, ld] (NumPy float64), mask uint8 [m] or None -> the dict of TrajectoryEngine.corridor_drivers
    with R as the only row axis, plus 'mean_abs' / 'factor_mean_abs' (mean |x|, the scale of the bound on a mean) and 'cond': the condition number of every row's factor correlation matrix (NaN without one)."""
    factors, values = np.asarray(factors, dtype=np.float64), np.asarray(values, dtype=np.float64)
    F, R = factors.shape[0], values.shape[0]
    m = min(factors.shape[1], values.shape[1]) if m is None else int(m)
    x, y = factors[:, :m], values[:, :m]
    masked = np.zeros(m, dtype=bool) if mask is None else np.asarray(mask)[:m] != 0
    fin = np.isfinite(x).all(axis=0)
    base = ~masked & fin
    out = {"m": m, "n_base": int(base.sum()), "n_masked": int(masked.sum()), "n_factor_non_finite": int((~masked & ~fin).sum())}
    xb = x[:, base]
    some = out["n_base"] > 0
    out["factor_mean"] = xb.mean(axis=1) if some else np.full(F, NAN)
    out["factor_std"] = np.sqrt(((xb - out["factor_mean"][:, None]) ** 2).mean(axis=1)) if some else np.full(F, NAN)
    out["factor_mean_abs"] = np.abs(xb).mean(axis=1) if some else np.full(F, NAN)
    out["factor_min"] = xb.min(axis=1) if some else np.full(F, NAN)
    out["factor_max"] = xb.max(axis=1) if some else np.full(F, NAN)
    out["factor_constant"] = (out["factor_min"] == out["factor_max"]) if some else np.zeros(F, dtype=bool)
    out["count"] = np.zeros(R, dtype=np.int64)
    for k in ("mean", "mean_abs", "std", "min", "max", "r2", "pivot_min", "cond"):
        out[k] = np.full(R, NAN)
    out["constant"], out["regression_ok"] = np.zeros(R, dtype=bool), np.zeros(R, dtype=bool)
    out["pearson"] = np.full((R, F), NAN)
    out["src"] = np.full((R, F), NAN) if regression else None
    for r in range(R):
        pop = base & np.isfinite(y[r])
        n = int(pop.sum())
        out["count"][r] = n
        if n == 0:
            continue
        yr, xr = y[r, pop], x[:, pop]
        out["mean"][r] = yr.mean()
        out["mean_abs"][r] = np.abs(yr).mean()
        out["std"][r] = np.sqrt(((yr - yr.mean()) ** 2).mean())
        out["min"][r], out["max"][r] = yr.min(), yr.max()
        out["constant"][r] = yr.min() == yr.max()
        if n < 2:
            continue
        varies = xr.min(axis=1) != xr.max(axis=1)
        xc = xr - xr.mean(axis=1)[:, None]
        yc = yr - yr.mean()
        sxx, syy, sxy = (xc * xc).sum(axis=1), float((yc * yc).sum()), xc @ yc
        with np.errstate(all="ignore"):
            rfy = sxy / (np.sqrt(sxx) * np.sqrt(syy))
        if not out["constant"][r]:
            out["pearson"][r, varies] = rfy[varies]
        if not regression:
            continue
        use = np.flatnonzero(varies)
        with np.errstate(all="ignore"):
            Rff = (xc[use] @ xc[use].T) / np.outer(np.sqrt(sxx[use]), np.sqrt(sxx[use]))
        np.fill_diagonal(Rff, 1.0)
        L, low = _cholesky(Rff)
        out["pivot_min"][r] = low
        out["regression_ok"][r] = L is not None
        if len(use):
            out["cond"][r] = np.linalg.cond(Rff)
        if L is None or out["constant"][r]:
            continue
        beta = np.linalg.solve(L.T, np.linalg.solve(L, rfy[use]))
        out["src"][r, use] = beta
        out["r2"][r] = float(beta @ rfy[use])
    return out


# the rows with a meaning of their own in make_case (where the shape has room for them)
ROW_ALL_NAN, ROW_ONE, ROW_CONSTANT, ROW_ZEROS, ROW_FACTOR_CONSTANT, ROW_COUNT_F = 1, 2, 4, 5, 6, 8
SENTINEL = 12345.0


def make_case(m, ld, F, R, seed, affine=False):
    """(factors [F, ld], values [R, ld], mask [m]) of a test: about 30 % NaN and some +-inf in `values`, 10 % of the mask bytes
    set, one factor with a NaN; the padding behind m holds a sentinel.  From five factors and nine rows on: factor 1 is
    correlated with factor 0 at about 0.57, factor 2 is constant on the base population, factor 3 takes three values (it is
    constant on the population of ROW_FACTOR_CONSTANT alone), factor 4 lies 1e4 standard deviations from zero; the rows
    ROW_* are an all-NaN row, a population of one, a constant row, a row constant as -0.0 / +0.0 and a row with as many columns as
    factors in its regression (count = F - 1: factor 2 is constant).
    affine: factor 4 is an affine image of factor 1.  The condition number of the factor correlation matrix over the base
    population (factor 2 left out) is asserted to be at most 10 unless the pair is affine."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(F, ld))
    full = F >= 5 and R >= 9 and m >= 64
    if full:
        x[1] = 0.57 * x[0] + np.sqrt(1.0 - 0.57 ** 2) * x[1]
        x[2] = 2.5
        x[3] = np.arange(ld) % 3 - 1.0
        x[4] = 1e4 + x[4]
        if affine:
            x[4] = 3.0 - 2.0 * x[1]
    if m > 5:
        x[0, 5] = NAN
    mask = (rng.random(m) < 0.1).astype(np.uint8) * 4
    base = (mask == 0) & np.isfinite(x[:, :m]).all(axis=0)
    coef = rng.normal(size=(R, F)) * (rng.random((R, F)) < 0.5)
    clean = np.where(np.isfinite(x), x, 0.0)
    spread = np.where(clean.std(axis=1) > 0, clean.std(axis=1), 1.0)
    y = coef @ ((clean - clean.mean(axis=1)[:, None]) / spread[:, None]) + 0.5 * rng.normal(size=(R, ld)) + 100.0 * np.arange(R)[:, None]
    y[rng.random((R, ld)) < 0.3] = NAN
    y[rng.random((R, ld)) < 0.01] = np.inf
    y[rng.random((R, ld)) < 0.01] = -np.inf
    if full:
        at = np.flatnonzero(base)
        y[ROW_ALL_NAN] = NAN
        y[ROW_ONE] = NAN
        y[ROW_ONE, at[len(at) // 2]] = 1.25
        y[ROW_CONSTANT, np.isfinite(y[ROW_CONSTANT])] = -3.5
        y[ROW_ZEROS, np.isfinite(y[ROW_ZEROS])] = 0.0
        y[ROW_ZEROS, ::2] = np.where(np.isfinite(y[ROW_ZEROS, ::2]), -0.0, y[ROW_ZEROS, ::2])
        y[ROW_FACTOR_CONSTANT, x[3] != 0.0] = NAN
        keep = at[3:3 + F - 1]   # as many columns as factors that vary (factor 2 does not): a singular regression
        row = np.full(ld, NAN)
        row[keep] = rng.normal(size=F - 1)
        y[ROW_COUNT_F] = row
    x[:, m:] = SENTINEL
    y[:, m:] = SENTINEL
    if full and not affine:
        use = [f for f in range(F) if f != 2]
        assert np.linalg.cond(np.corrcoef(x[use][:, :m][:, base])) <= 10.0
    return np.ascontiguousarray(x), np.ascontiguousarray(y), mask


def src_bound(cond):
    """The bound on src and r2 of a row whose factor correlation matrix has condition number `cond`: that of pearson (1e-12)
    times the condition number with a margin of 10 - 1e-10 at the condition number 10 the generator admits."""
    return 1e-12 * 10.0 * np.maximum(cond, 10.0)
