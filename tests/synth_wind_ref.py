"""The wind table of erpl_mc_synth_wind (include/erpl_mc.h) restated on the host in np.longdouble, and the magnitude
E that bounds what a correct fp64 evaluation of it may differ by.

    wind[i][c][s] = base[i][c] + scale[i] * mean_c[s] + t_i
    t_0 = sigma[0] f_c z,  t_i = rho[i] t_{i-1} + innov[i] f_c z,  f = (1, 1, 0.3),  mean_2 = 0,  z = normals[i][c][s]

Relative error is the wrong measure of such a table: mean + t cancels, so a correct evaluation reaches 5e-12 relative
at 1024 knots.  What a correct evaluation is free to choose - the order of the mean-wind sum, FMA contraction, and (in
flatten._ar1_profiles, as in the reference) carrying `wind - mean` from knot to knot instead of t - costs a few roundings
of the magnitudes that enter a knot, and rho carries them on to the next one.  E is that running magnitude:

    mean_i = |base[i][c]| + scale[i] |mean_c[s]|
    M_0 = |sigma[0] f_c z_0|,        M_i = rho[i] M_{i-1} + |innov[i] f_c z_i|
    E_0 = mean_0 + M_0,              E_i = rho[i] E_{i-1} + mean_i + M_i          (0 <= rho <= 1)

and the tolerance of an fp64 table is TOL * eps64 * E, element by element and absolute.  A plain fp64 evaluation of the
formula stays at or below 1.8 eps E of flatten._ar1_profiles (CSV K = 6, power law K = 100, K = 1024 with rho = 0.78,
K = 2; n = 300 each); 8 is the margin over that, a condition on the kernel and not a figure fitted to it.
tests/test_synth_wind_ref.py pins this file to flatten._ar1_profiles, which tests/test_host.py pins to the reference's
captured tables.  Host only, NumPy only; no product code imports it."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
TOL = 8.0            # fp64 device table against `reference`: |got - ref| <= TOL * EPS * E
TOL_HOST = 2.0       # `reference` against flatten._ar1_profiles
COMP = (1.0, 1.0, 0.3)

LD = np.longdouble
OK, ERR_INVALID = 0, -1      # ERPL_OK, ERPL_ERR_INVALID of include/erpl_mc.h


def _inputs(normals, sigma, rho, innov, base, scale, mean_u, mean_v, dtype):
    sigma, rho, innov, scale = (np.asarray(v, dtype=np.float64).astype(dtype) for v in (sigma, rho, innov, scale))
    K = sigma.shape[0]
    mean_u, mean_v = np.asarray(mean_u, dtype=np.float64), np.asarray(mean_v, dtype=np.float64)
    n = mean_u.shape[0]
    z = np.asarray(normals, dtype=np.float64).reshape(K, 3, n).astype(dtype)
    base = np.zeros((K, 3), dtype=dtype) if base is None else np.asarray(base, dtype=np.float64).reshape(K, 3).astype(dtype)
    mean = np.stack([mean_u, mean_v, np.zeros(n)]).astype(dtype)
    # the constants as the fp64 kernel holds them: 0.3 is the double nearest to 0.3, not the long double
    f = np.array(COMP, dtype=np.float64).astype(dtype)[:, None]
    if rho.shape != (K,) or innov.shape != (K,) or scale.shape != (K,) or mean_v.shape != (n,):
        raise ValueError("sigma, rho, innov, scale: [K]; mean_u, mean_v: [n]")
    return K, n, z, sigma, rho, innov, base, scale, mean, f


def _evaluate(dtype, normals, sigma, rho, innov, base, scale, mean_u, mean_v):
    K, n, z, sigma, rho, innov, base, scale, mean, f = _inputs(normals, sigma, rho, innov, base, scale, mean_u, mean_v, dtype)
    out = np.empty((K, 3, n), dtype=dtype)
    t = np.zeros((3, n), dtype=dtype)
    for i in range(K):
        t = (sigma[0] * f) * z[0] if i == 0 else rho[i] * t + (innov[i] * f) * z[i]
        out[i] = (base[i][:, None] + scale[i] * mean) + t
    return out


def reference(normals, sigma, rho, innov, base, scale, mean_u, mean_v):
    """The table [K, 3, n] in np.longdouble.  normals: [K, 3, n] (or [3 K, n]); sigma, rho, innov, scale: [K]; base: [K, 3]
    or None; mean_u, mean_v: [n].  rho[0] and innov[0] are not read."""
    return _evaluate(LD, normals, sigma, rho, innov, base, scale, mean_u, mean_v)


def evaluate_fp64(normals, sigma, rho, innov, base, scale, mean_u, mean_v):
    """The same formula in plain float64, operation for operation as the header writes it (no FMA): one of the
    evaluations the tolerance has to admit."""
    return _evaluate(np.float64, normals, sigma, rho, innov, base, scale, mean_u, mean_v)


def bound(normals, sigma, rho, innov, base, scale, mean_u, mean_v):
    """E [K, 3, n] (float64) of the module docstring."""
    K, n, z, sigma, rho, innov, base, scale, mean, f = _inputs(normals, sigma, rho, innov, base, scale, mean_u, mean_v, LD)
    if not (np.all(rho[1:] >= 0) and np.all(rho[1:] <= 1)):
        raise ValueError("the bound holds for 0 <= rho <= 1")
    E = np.empty((K, 3, n), dtype=LD)
    M = np.zeros((3, n), dtype=LD)
    for i in range(K):
        mean_i = np.abs(base[i])[:, None] + scale[i] * np.abs(mean)
        if i == 0:
            M = np.abs(sigma[0] * f * z[0])
            E[0] = mean_i + M
        else:
            M = rho[i] * M + np.abs(innov[i] * f * z[i])
            E[i] = rho[i] * E[i - 1] + mean_i + M
    return E.astype(np.float64)


def excess(got, ref, E):
    """max over the table of |got - ref| / (eps E), with 0 / 0 = 0 and x / 0 = inf: compare with TOL."""
    d = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - np.asarray(ref).astype(LD)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / (EPS * np.asarray(E, dtype=np.float64)))
    if np.isnan(r).any():
        return float("inf")
    return float(r.max()) if r.size else 0.0


def knot_inputs(seed, K):
    """Hand-made per-knot constants that differ at every knot, so that an index slip moves the result: sigma in [0.5, 3],
    rho in [0.05, 0.95] with rho[0] = 0, innov in [0.1, 2], scale in [0, 3], base [K, 3] in [-20, 20]."""
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(0.5, 3.0, K)
    rho = rng.uniform(0.05, 0.95, K)
    rho[0] = 0.0
    innov = rng.uniform(0.1, 2.0, K)
    scale = rng.uniform(0.0, 3.0, K)
    base = rng.uniform(-20.0, 20.0, (K, 3))
    return sigma, rho, innov, scale, base


def sample_inputs(seed, K, n):
    """Standard normals [K, 3, n] and mean-wind rows [n] (up to +-5 m/s, both signs)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, 3, n)), rng.uniform(-5.0, 5.0, n), rng.uniform(-5.0, 5.0, n)
