"""tests/density_w_ref.py - the NumPy restatement of erpl_mc_impact_density_weighted - against scipy.stats.gaussian_kde(weights=),
np.quantile(weights=, method="inverted_cdf") and the unweighted rule on repeated columns.  No GPU, no library."""
import math

import numpy as np
import pytest

import density_w_ref as R


def cloud(kind, m, seed):
    """tests/test_gpu_density.py's clouds: 'gauss' = a correlated Gaussian away from the origin, 'mix' = two clusters."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((2, m))
    if kind == "gauss":
        x = 1500.0 + 300.0 * z[0]
        y = -800.0 + 120.0 * (0.9 * z[0] + math.sqrt(1.0 - 0.81) * z[1])
    else:
        first = rng.random(m) < 0.6
        first[:2] = (True, False)
        x = np.where(first, -400.0 + 80.0 * z[0], 700.0 + 150.0 * z[0])
        y = np.where(first, 250.0 + 120.0 * z[1], -300.0 + 60.0 * z[1])
    return x, y


def reweight_like(m, seed, scale=40):
    """floor(2^scale exp(l - l_max)), l = -Exp(4): what erpl_mc_reweight writes for a strongly changed law (some zeros)."""
    rng = np.random.default_rng(seed + 5)
    l = -rng.exponential(4.0, m)
    return np.floor(np.ldexp(np.exp(l - l.max()), scale)).astype(np.int64)


CLOUDS = [("gauss", 63, 1), ("mix", 257, 2), ("gauss", 1025, 3), ("mix", 4099, 4)]


@pytest.mark.parametrize("kind,m,seed", CLOUDS)
def test_ess_and_bandwidth_are_scipys(kind, m, seed):
    stats = pytest.importorskip("scipy.stats")
    x, y = cloud(kind, m, seed)
    W = reweight_like(m, seed)
    keep = W > 0
    assert (~keep).sum() < m
    mean, cov, sum_w2, ess = R.moments(x[keep], y[keep], W[keep])
    kde = stats.gaussian_kde(np.vstack([x[keep], y[keep]]), weights=W[keep].astype(np.float64))
    e_ess = abs(ess / kde.neff - 1.0)
    Hm = R.bandwidth(cov, ess)
    e_h = np.abs(Hm / kde.covariance - 1.0).max()
    print(f"{kind} m={m}: ess {ess:.6g} rel err {e_ess:.3g}, H rel err {e_h:.3g}")
    assert e_ess <= 1e-12 and e_h <= 1e-12
    # the density itself is scipy's on body nodes (the definition, not the rounding)
    gx, gy = np.meshgrid(np.linspace(x.min(), x.max(), 12), np.linspace(y.min(), y.max(), 9), indexing="ij")
    ref = kde(np.vstack([gx.ravel(), gy.ravel()]))
    got = R.density(gx.ravel(), gy.ravel(), x[keep], y[keep], W[keep], Hm)
    body = ref >= 1e-12 * ref.max()
    assert body.sum() > 20 and np.abs(got[body] / ref[body] - 1.0).max() <= 1e-9


@pytest.mark.parametrize("kind,m,seed", CLOUDS)
def test_thresholds_are_numpys_weighted_inverted_cdf(kind, m, seed):
    x, y = cloud(kind, m, seed)
    for W in (reweight_like(m, seed), np.full(m, 1 << 20, dtype=np.int64),
              np.random.default_rng(seed).integers(0, 4, m).astype(np.int64)):
        keep = W > 0
        mean, cov, _, ess = R.moments(x[keep], y[keep], W[keep])
        f = R.density(x[keep], y[keep], x[keep], y[keep], W[keep], R.bandwidth(cov, ess))
        levels = [0.5, 0.9, 0.99, 0.25, 0.999]
        t = R.thresholds(f, W[keep], levels)
        sum_w = int(W[keep].astype(object).sum())
        for p, tk in zip(levels, t):
            want = np.quantile(f, 1.0 - p, weights=W[keep], method="inverted_cdf")
            assert np.float64(tk).view(np.int64) == np.float64(want).view(np.int64), (p, tk, want)
            c = R.content_w(f, W[keep], tk)
            assert c >= p * sum_w and c <= sum_w, (p, c, sum_w)


@pytest.mark.parametrize("kind,m,seed", CLOUDS)
def test_small_integer_weights_are_repeated_columns(kind, m, seed):
    x, y = cloud(kind, m, seed)
    W = np.random.default_rng(seed + 9).integers(0, 4, m).astype(np.int64)
    keep = W > 0
    xr, yr = np.repeat(x, W), np.repeat(y, W)
    Hm = [[0.04 * x.var(), 0.01 * x.std() * y.std()], [0.01 * x.std() * y.std(), 0.04 * y.var()]]
    gx, gy = np.meshgrid(np.linspace(x.min(), x.max(), 33), np.linspace(y.min(), y.max(), 17), indexing="ij")
    mean = [xr.mean(), yr.mean()]
    a = R.density(gx.ravel(), gy.ravel(), x[keep], y[keep], W[keep], Hm, mean)
    b = R.density_unweighted(gx.ravel(), gy.ravel(), xr, yr, Hm, mean)
    err = np.abs(a - b).max() / b.max()
    print(f"{kind} m={m}: weighted against repeated columns, worst |diff| / peak {err:.3g}")
    assert err <= 1e-13
    # the weighted moments are those of the repeated columns, and the zone weights their counts - exactly
    mw, cw, _, _ = R.moments(x[keep], y[keep], W[keep])
    assert np.allclose(mw, mean, rtol=1e-13) and R.scaled(W[keep])[3] == len(xr)
    tri = np.array([[x.min(), y.min()], [x.max(), y.min()], [np.median(x), y.max()]])
    assert R.zone_weight(tri, x, y, W) == int(R.crossing(tri[:, 0], tri[:, 1], xr, yr).sum()) > 0


def test_population_order_and_scaling():
    x = np.array([1.0, np.nan, 2.0, 3.0, 4.0, np.inf])
    y = np.array([0.0, 0.0, np.nan, 1.0, 2.0, 1.0])
    W = np.array([5, 0, 7, 0, 1 << 40, 3], dtype=np.int64)
    mask = np.array([0, 9, 0, 0, 0, 1], dtype=np.uint8)
    counted, n_masked, n_bad, n_zero = R.population(x, y, W, mask)
    assert list(counted) == [True, False, False, False, True, False] and (n_masked, n_bad, n_zero) == (2, 1, 1)
    w, s_d, K, sum_w, max_w = R.scaled(W[counted])
    assert K == 41 and max_w == 1 << 40 and sum_w == (1 << 40) + 5 and list(w) == [5 * 2.0 ** -41, 0.5]
    assert s_d == math.ldexp(float(sum_w), -41)
    assert R.rw_q(1) == 52 and R.rw_q(1024) == 52 and R.rw_q(1025) == 51 and R.rw_q(4096) == 50
    assert R.target_rank(0.5, 10) == 5 and R.target_rank(0.999999, 10) == 1 and R.target_rank(1e-9, 10) == 10
