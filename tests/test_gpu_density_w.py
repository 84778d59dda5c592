"""erpl_mc_impact_density_weighted on the device: the weighted kernel density at the nodes and at the samples against an
extended-precision sum, and what has to hold exactly - the nodes, the counts, sum_w, max_w, the zone weights, the weighted
thresholds and their contents, the peak - plus equal weights against erpl_mc_impact_density, a permutation of the columns,
the same bytes twice, the refusal of a weight outside 0 .. 2^Q, the degenerate clouds and one flown run against
erpl_mc_reweight and against a run flown under the target law.

The density tolerance is MEASURED, the rule of tests/test_gpu_density.py restated with weights.  Truth is the direct
quadratic form in np.longdouble with the H the call returned.  Two float64 formulations are compared against it - the direct
quadratic form in NumPy, and scipy.stats.gaussian_kde(weights=) evaluating with that H - and nodes fall into three classes
by truth / peak: body >= 1e-12, tail [1e-280, 1e-12), dead < 1e-280.  In body and tail the device's worst relative error may
be at most 4 x the worse of the two formulations' errors in that class plus (m + 64) * 2^-53; dead nodes must be
<= 1e-279 x peak.  Every case prints its figures (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import density_w_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
RX, RY = _abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def cloud(kind, m, seed):
    """m impact points: 'gauss' = a correlated Gaussian (rho = 0.9) away from the origin, 'mix' = two clusters."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((2, m))
    if kind == "gauss":
        x = 1500.0 + 300.0 * z[0]
        y = -800.0 + 120.0 * (0.9 * z[0] + math.sqrt(1.0 - 0.81) * z[1])
    else:
        first = rng.random(m) < 0.6
        first[:2] = (True, False)   # both clusters from three points on (never all on a line with the third)
        x = np.where(first, -400.0 + 80.0 * z[0], 700.0 + 150.0 * z[0])
        y = np.where(first, 250.0 + 120.0 * z[1], -300.0 + 60.0 * z[1])
    return x, y


def summary_of(x, y, junk=False, seed=0):
    """(summary [16, n], mask [n] or None, the indices of the m points): with junk the m points are interleaved, in their
    order, with masked samples and with NaN / +-inf entries in either row."""
    m = len(x)
    if not junk:
        summ = np.zeros((_abi.SUMMARY_DIM, m))
        summ[RX], summ[RY] = x, y
        return summ, None, np.arange(m)
    rng = np.random.default_rng(seed + 77)
    n = m + max(7, m // 3)
    at = np.sort(rng.choice(n, size=m, replace=False))
    summ = np.zeros((_abi.SUMMARY_DIM, n))
    summ[RX], summ[RY] = rng.normal(0.0, 1e4, n), rng.normal(0.0, 1e4, n)   # what a wrong population would pick up
    mask = np.zeros(n, dtype=np.uint8)
    other = np.setdiff1d(np.arange(n), at)
    for k, i in enumerate(other):
        how = k % 5
        if how == 0:
            mask[i] = 1 + k % 63
        elif how == 1:
            summ[RX, i] = np.nan
        elif how == 2:
            summ[RY, i] = np.inf
        elif how == 3:
            summ[RX, i] = -np.inf
            mask[i] = 4
        else:
            summ[RY, i] = np.nan
    summ[RX, at], summ[RY, at] = x, y
    return summ, mask, at


def weights_of(kind, m, seed):
    """'rw': floor(2^40 exp(l - l_max)), l = -Exp(4) - what erpl_mc_reweight writes, with some zeros from about a thousand
    points on; 'equal': every weight 2^33 + 5; 'small': integers 0 .. 3."""
    rng = np.random.default_rng(seed + 5)
    if kind == "rw":
        l = -rng.exponential(4.0, m)
        return np.floor(np.ldexp(np.exp(l - l.max()), 40)).astype(np.int64)
    if kind == "equal":
        return np.full(m, (1 << 33) + 5, dtype=np.int64)
    W = rng.integers(0, 4, m).astype(np.int64)
    W[:3] = (1, 2, 3)   # at least three points of both clusters count
    return W


def weight_row(W, at, n):
    """The [n] row: W at the m points, admissible weights that must not count everywhere else."""
    row = np.full(n, 12345, dtype=np.int64)
    row[at] = W
    return row


def dev(engine, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def truth_ld(qx, qy, px, py, W, Hm):
    """sum_i W_i exp(-(q - p_i)' H^-1 (q - p_i) / 2) / (sum_w 2 pi sqrt(det H)) in long double, for the query points q."""
    hxx, hxy, hyy = LD(Hm[0][0]), LD(Hm[0][1]), LD(Hm[1][1])
    det = hxx * hyy - hxy * hxy
    a, b, c = hyy / det, -hxy / det, hxx / det
    qx, qy, px, py = (np.asarray(v, dtype=np.float64).astype(LD) for v in (qx, qy, px, py))
    w = np.asarray(W, dtype=np.int64).astype(LD)
    out = np.zeros(len(qx), dtype=LD)
    step = max(1, 2_000_000 // max(len(qx), 1))
    for s in range(0, len(px), step):
        dx, dy = qx[:, None] - px[None, s:s + step], qy[:, None] - py[None, s:s + step]
        out += (w[None, s:s + step] * np.exp(LD(-0.5) * (a * dx * dx + LD(2) * b * dx * dy + c * dy * dy))).sum(axis=1)
    return out / (w.sum() * LD(2) * LD(np.pi) * np.sqrt(det))


def direct_f64(qx, qy, px, py, W, Hm):
    hxx, hxy, hyy = Hm[0][0], Hm[0][1], Hm[1][1]
    det = hxx * hyy - hxy * hxy
    a, b, c = hyy / det, -hxy / det, hxx / det
    w = np.asarray(W, dtype=np.float64)
    out = np.zeros(len(qx))
    step = max(1, 2_000_000 // max(len(qx), 1))
    for s in range(0, len(px), step):
        dx, dy = qx[:, None] - px[None, s:s + step], qy[:, None] - py[None, s:s + step]
        out += (w[None, s:s + step] * np.exp(-0.5 * (a * dx * dx + 2.0 * b * dx * dy + c * dy * dy))).sum(axis=1)
    return out / (w.sum() * 2.0 * np.pi * np.sqrt(det))


def scipy_f64(qx, qy, px, py, W, Hm):
    """scipy.stats.gaussian_kde(weights=W) evaluating with the H of the call: its covariance replaced by Hm as
    _compute_covariance would set it.  One point has no covariance for scipy to start from: its formulation restated
    (density_w_ref.density)."""
    stats = pytest.importorskip("scipy.stats")
    if len(px) < 2:
        return R.density(qx, qy, px, py, W, Hm)
    kde = stats.gaussian_kde(np.vstack([px, py]), weights=np.asarray(W, dtype=np.float64), bw_method=1.0)
    kde.covariance = np.asarray(Hm, dtype=np.float64)
    kde.cho_cov = np.linalg.cholesky(kde.covariance).astype(np.float64)
    kde.log_det = 2 * np.log(np.diag(kde.cho_cov * np.sqrt(2 * np.pi))).sum()
    return kde(np.vstack([qx, qy]))


def judge(label, got, qx, qy, px, py, W, Hm):
    """The measured-tolerance comparison of the module docstring for the device values `got` at the query points."""
    assert np.finfo(LD).nmant == 63   # x86-64 extended precision: a long double that is a double would be no truth
    m = len(px)
    t = truth_ld(qx, qy, px, py, W, Hm)
    refs = [direct_f64(qx, qy, px, py, W, Hm), scipy_f64(qx, qy, px, py, W, Hm)]
    peak = t.max()
    ratio = t / peak
    classes = (("body", ratio >= LD(1e-12)), ("tail", (ratio >= LD(1e-280)) & (ratio < LD(1e-12))), ("dead", ratio < LD(1e-280)))
    assert sum(int(sel.sum()) for _, sel in classes) == len(t)   # no node is left out
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all() and (got >= 0.0).all()
    for name, sel in classes:
        if not sel.any():
            continue
        if name == "dead":
            worst = float(got[sel].max() / float(peak))
            print(f"{label} dead: {int(sel.sum())} nodes, device max / peak {worst:.3g}")
            assert worst <= 1e-279
            continue
        rel = lambda v: float((np.abs(v[sel].astype(LD) - t[sel]) / t[sel]).max())   # noqa: E731
        e_dev, e_ref = rel(got), [rel(r) for r in refs]
        bound = 4.0 * max(e_ref) + (m + 64) * U
        print(f"{label} {name}: {int(sel.sum())} nodes, device {e_dev:.3g}, direct {e_ref[0]:.3g}, scipy {e_ref[1]:.3g}, "
              f"bound {bound:.3g}")
        assert e_dev <= bound, (label, name, e_dev, e_ref, bound)


def same_bytes(a, b):
    """Two results of one call: nested dicts / lists of numbers and arrays, the doubles bit for bit (a NaN equals a NaN)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bytes(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bytes(u, v) for u, v in zip(a, b))
    if torch.is_tensor(a):
        a, b = a.cpu().numpy(), b.cpu().numpy()
    if isinstance(a, (np.ndarray, float)):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


def wide_ranges(x, y):
    """Ranges 1.5 spans beyond the cloud: body, tail and (for the larger clouds, whose bandwidth is small) dead nodes."""
    sx, sy = x.max() - x.min(), y.max() - y.min()
    return (x.min() - 1.5 * sx, x.max() + 1.5 * sx), (y.min() - 1.5 * sy, y.max() + 1.5 * sy)


def zones_of(x, y):
    """A triangle over the middle of the cloud and a box around its upper right part."""
    cx, cy, sx, sy = np.median(x), np.median(y), x.std(), y.std()
    return [np.array([[cx - sx, cy - sy], [cx + sx, cy - 0.5 * sy], [cx, cy + sy]]),
            np.array([[cx, cy], [cx + 9 * sx, cy], [cx + 9 * sx, cy + 9 * sy], [cx, cy + 9 * sy]])]


# (label, cloud, m, nodes, weights)
CASES = [("m3", "mix", 3, (64, 48), "equal"), ("m63", "gauss", 63, (64, 48), "rw"), ("m64", "mix", 64, (64, 48), "small"),
         ("m65", "gauss", 65, (64, 48), "rw"), ("m257", "mix", 257, (64, 48), "rw"), ("m1025", "gauss", 1025, (64, 48), "small"),
         ("m1025-rw", "mix", 1025, (64, 48), "rw"), ("m4099", "gauss", 4099, (64, 48), "rw"), ("m4099-equal", "mix", 4099, (64, 48), "equal"),
         ("3x5", "gauss", 257, (3, 5), "small"), ("255x257", "gauss", 257, (255, 257), "rw")]


@pytest.mark.parametrize("label,kind,m,nodes,wkind", CASES, ids=[c[0] for c in CASES])
def test_weighted_density_at_the_nodes_and_at_the_samples(engine, label, kind, m, nodes, wkind):
    x, y = cloud(kind, m, 1000 + m)
    summ, mask, at = summary_of(x, y, True, seed=m)
    n = summ.shape[1]
    W_all = weights_of(wkind, m, m)
    wrow = weight_row(W_all, at, n)
    keep = W_all > 0
    px, py, W = x[keep], y[keep], W_all[keep]
    counted = np.zeros(n, dtype=bool)
    counted[at[keep]] = True
    ranges = wide_ranges(x, y)
    zones = zones_of(x, y)
    out = engine.impact_density_weighted(dev(engine, summ), dev(engine, wrow), dev(engine, mask), nodes=nodes, ranges=ranges,
                                         zones=zones, sample_density=True)
    # exact: the population in the order of the header, the integer sums
    want_counted, n_masked, n_bad, n_zero = R.population(summ[RX], summ[RY], wrow, mask)
    assert np.array_equal(want_counted, counted)
    w, s_d, K, sum_w, max_w = R.scaled(W)
    print(f"{label}: count {out['count']} of {m}, n_zero {out['n_zero']}, K {K}, ess {out['ess']:.6g}")
    assert (out["count"], out["n_masked"], out["n_non_finite"], out["n_zero"]) == (int(keep.sum()), n_masked, n_bad, n_zero)
    assert n_zero == int((~keep).sum()) and (out["sum_w"], out["max_w"]) == (sum_w, max_w) and out["solid"]
    # 1e-12: the moments, ess and H against the restatement
    mean, cov, sum_w2, ess = R.moments(px, py, W)
    Hm = out["bandwidth_matrix"]
    want_h = R.bandwidth(cov, ess)
    scale = [math.sqrt(cov[0, 0]), math.sqrt(cov[1, 1])]
    for k in range(2):
        assert abs(out["mean"][k] - mean[k]) <= 1e-12 * (abs(mean[k]) + scale[k])
    assert abs(out["ess"] - ess) <= 1e-12 * ess and abs(out["sum_w2"] - sum_w2) <= 1e-12 * sum_w2
    for i, j in ((0, 0), (0, 1), (1, 1)):
        assert abs(out["covariance"][i][j] - cov[i, j]) <= 1e-12 * scale[i] * scale[j]
        assert abs(Hm[i][j] - want_h[i, j]) <= 1e-12 * math.sqrt(want_h[i, i] * want_h[j, j])
    # exact: the nodes are np.linspace of the returned range, which is the explicit one
    assert out["ranges"] == (tuple(float(v) for v in ranges[0]), tuple(float(v) for v in ranges[1]))
    assert np.array_equal(bits(out["grid_x"]), bits(np.linspace(*out["ranges"][0], nodes[0])))
    assert np.array_equal(bits(out["grid_y"]), bits(np.linspace(*out["ranges"][1], nodes[1])))
    gx, gy = np.meshgrid(out["grid_x"], out["grid_y"], indexing="ij")   # x-major
    dens = out["density"]
    assert dens.shape == nodes
    judge(label + " grid", dens.ravel(), gx.ravel(), gy.ravel(), px, py, W, Hm)
    # exact: the peak and its node; the mass to 1e-12
    assert out["peak"] == dens.max() and out["peak_node"] == tuple(int(v) for v in np.unravel_index(np.argmax(dens), nodes))
    cell = ((ranges[0][1] - ranges[0][0]) / (nodes[0] - 1)) * ((ranges[1][1] - ranges[1][0]) / (nodes[1] - 1))
    assert abs(out["grid_mass"] - dens.sum() * cell) <= 1e-12 * dens.sum() * cell
    # the samples: NaN exactly where a sample is not counted; every counted one against the truth
    row = out["sample_density"].cpu().numpy()
    assert np.isnan(row[~counted]).all() and np.isfinite(row[counted]).all()
    f = row[counted]
    judge(label + " samples", f, px, py, px, py, W, Hm)
    # exact: the thresholds are NumPy's weighted inverted-CDF quantiles of the device's own row, and their contents
    assert out["f_min"] == f.min() and out["f_max"] == f.max()
    for k, p in enumerate(out["levels"]):
        want_t = np.quantile(f, 1.0 - p, weights=W, method="inverted_cdf")
        assert bits(out["thresholds"][k]) == bits(want_t), (k, p, out["thresholds"][k], want_t)
        assert out["thresholds"][k] == R.thresholds(f, W, [p])[0]
        assert out["content_w"][k] == R.content_w(f, W, out["thresholds"][k]) and out["content_w"][k] >= p * sum_w
    # exact: the zone weights against NumPy int64; the squared scaled weights inside to 1e-12
    for z, poly in zip(out["zones"], zones):
        inside = R.crossing(poly[:, 0], poly[:, 1], px, py)
        assert z["weight"] == int(W[inside].sum()) == R.zone_weight(poly, px, py, W)
        a2 = float((w[inside] * w[inside]).sum())
        assert abs(z["a2"] - a2) <= 1e-12 * sum_w2
    assert out["zones"][0]["weight"] <= sum_w and (m < 63 or out["zones"][0]["weight"] > 0)


def test_one_point_with_a_bandwidth_matrix(engine):
    Hm = [[4.0, 1.5], [1.5, 2.25]]
    summ = np.zeros((_abi.SUMMARY_DIM, 4))
    summ[RX], summ[RY] = [7.0, 10.5, np.nan, 3.0], [1.0, -2.25, 0.0, 3.0]
    mask = np.array([3, 0, 0, 0], dtype=np.uint8)
    wrow = np.array([5, 7, 9, 0], dtype=np.int64)
    out = engine.impact_density_weighted(dev(engine, summ), dev(engine, wrow), dev(engine, mask), nodes=(9, 7), bandwidth=Hm,
                                         sample_density=True)
    assert (out["count"], out["n_masked"], out["n_non_finite"], out["n_zero"]) == (1, 1, 1, 1)
    assert out["solid"] and out["bandwidth_matrix"] == Hm and out["mean"] == [10.5, -2.25] and (out["sum_w"], out["max_w"]) == (7, 7)
    assert out["ess"] == 1.0 and np.isnan(out["covariance"][0][0])   # no covariance of one point
    assert out["ranges"] == ((10.5 - 3 * 2.0, 10.5 + 3 * 2.0), (-2.25 - 3 * 1.5, -2.25 + 3 * 1.5))
    gx, gy = np.meshgrid(out["grid_x"], out["grid_y"], indexing="ij")
    judge("m1 matrix", out["density"].ravel(), gx.ravel(), gy.ravel(), np.array([10.5]), np.array([-2.25]), np.array([7]), Hm)
    row = out["sample_density"].cpu().numpy()
    norm = 1.0 / (2.0 * np.pi * math.sqrt(4.0 * 2.25 - 2.25))
    assert np.isnan(row[[0, 2, 3]]).all() and abs(row[1] - norm) <= 4 * U * norm and abs(out["norm"] * (7 / 8) - norm) <= 4 * U * norm
    assert out["thresholds"] == [row[1]] * 3 and out["content_w"] == [7] * 3
    assert out["peak_node"] == (4, 3) and out["peak"] == out["density"][4, 3]


def test_equal_weights_are_the_unweighted_map(engine):
    m, W0 = 1025, 3 << 20
    x, y = cloud("mix", m, 12)
    summ, mask, at = summary_of(x, y, True, seed=12)
    zones = zones_of(x, y)
    kw = dict(nodes=(64, 48), ranges=wide_ranges(x, y), zones=zones, sample_density=True)
    plain = engine.impact_density(dev(engine, summ), dev(engine, mask), **kw)
    wrow = np.full(summ.shape[1], W0, dtype=np.int64)
    out = engine.impact_density_weighted(dev(engine, summ), dev(engine, wrow), dev(engine, mask), **kw)
    assert out["count"] == plain["count"] == m and out["sum_w"] == m * W0 and out["solid"] and plain["solid"]
    assert abs(out["ess"] - m) <= 1e-12 * m
    sx, sy = math.sqrt(plain["covariance"][0][0]), math.sqrt(plain["covariance"][1][1])
    for k, s in enumerate((sx, sy)):
        assert abs(out["mean"][k] - plain["mean"][k]) <= 1e-12 * (abs(plain["mean"][k]) + s)
    for key in ("covariance", "bandwidth_matrix"):
        a, b = np.asarray(out[key]), np.asarray(plain[key])
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), key
    # the maps: both under the measured rule against the same truth form, each with its own H
    gx, gy = np.meshgrid(out["grid_x"], out["grid_y"], indexing="ij")
    ones = np.ones(m, dtype=np.int64)
    judge("equal weighted grid", out["density"].ravel(), gx.ravel(), gy.ravel(), x, y, ones, out["bandwidth_matrix"])
    judge("equal plain grid", plain["density"].ravel(), gx.ravel(), gy.ravel(), x, y, ones, plain["bandwidth_matrix"])
    judge("equal weighted samples", out["sample_density"].cpu().numpy()[at], x, y, x, y, ones, out["bandwidth_matrix"])
    # and each other: the two H agree to 1e-12 and an exponent is at most 745, so the maps agree to 1e-9 of the peak
    assert np.abs(out["density"] - plain["density"]).max() <= 1e-9 * plain["peak"]
    for zw, zp in zip(out["zones"], plain["zones"]):
        assert zw["weight"] == zp["inside"] * W0
    assert out["zones"][0]["weight"] > 0


def test_a_permutation_of_the_columns_and_the_same_bytes_twice(engine):
    m = 4099
    x, y = cloud("mix", m, 3)
    summ, mask, at = summary_of(x, y, True, seed=3)
    n = summ.shape[1]
    wrow = weight_row(weights_of("rw", m, 3), at, n)
    zones = zones_of(x, y)
    kw = dict(nodes=(64, 48), zones=zones, sample_density=True)
    a = engine.impact_density_weighted(dev(engine, summ), dev(engine, wrow), dev(engine, mask), **kw)
    b = engine.impact_density_weighted(dev(engine, summ), dev(engine, wrow), dev(engine, mask), **kw)
    assert same_bytes(a, b) and not same_bytes(a, dict(a, peak=a["peak"] * 2.0))   # everything, the doubles bit for bit
    assert a["n_zero"] > 0 and a["solid"]
    perm = np.random.default_rng(8).permutation(n)
    c = engine.impact_density_weighted(dev(engine, summ[:, perm]), dev(engine, wrow[perm]), dev(engine, mask[perm]), **kw)
    for key in ("count", "n_masked", "n_non_finite", "n_zero", "sum_w", "max_w"):
        assert a[key] == c[key], key
    assert [z["weight"] for z in a["zones"]] == [z["weight"] for z in c["zones"]] and a["zones"][0]["weight"] > 0
    assert abs(c["ess"] - a["ess"]) <= 1e-12 * a["ess"]


def test_a_weight_outside_the_bound_is_refused_with_its_column(engine):
    m = 300
    x, y = cloud("gauss", m, 4)
    summ, mask, at = summary_of(x, y, True, seed=4)
    n = summ.shape[1]
    Q = R.rw_q(n)
    assert Q == 52
    good = weight_row(weights_of("small", m, 4), at, n)
    good[at[7]] = 1 << Q   # the bound itself is admitted
    assert engine.impact_density_weighted(dev(engine, summ), dev(engine, good), dev(engine, mask), nodes=(8, 6))["max_w"] == 1 << Q
    s, k = dev(engine, summ), dev(engine, mask)
    spec = engine._defaults(_abi.ErplDensitySpec, "erpl_mc_impact_density_defaults")
    spec.nodes_x, spec.nodes_y = 8, 6
    for col, value in ((int(at[41]), -1), (int(at[200]), (1 << Q) + 1), (5, -(1 << 62))):
        bad = good.copy()
        bad[col] = value
        bad[n - 1] = -3 if col != n - 1 else value   # a later offender: the message names the lowest column
        with pytest.raises(_abi.ErplError, match=rf"weights\[{col}\]"):
            engine.impact_density_weighted(s, dev(engine, bad), k, nodes=(8, 6))
        # no output is written: the result, the host arrays and the caller's device row as they were
        res = _abi.ErplDensityW()
        C.memset(C.byref(res), 0xA5, C.sizeof(res))
        before = bytes(res)
        gx, gy, dens = np.full(512, -7.0), np.full(512, -7.0), np.full(48, -7.0)
        row = torch.full((n,), -7.0, dtype=torch.float64, device=engine.device)
        wt = dev(engine, bad)
        rc = engine.lib.erpl_mc_impact_density_weighted(engine._ctx, C.c_void_p(s.data_ptr()), C.c_void_p(k.data_ptr()),
                                                        C.c_void_p(wt.data_ptr()), n, C.byref(spec), C.c_void_p(gx.ctypes.data),
                                                        C.c_void_p(gy.ctypes.data), C.c_void_p(dens.ctypes.data), C.byref(res),
                                                        C.c_void_p(row.data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == -1 and f"weights[{col}]".encode() in engine.lib.erpl_mc_last_error()
        assert bytes(res) == before and (gx == -7.0).all() and (gy == -7.0).all() and (dens == -7.0).all() and bool((row == -7.0).all())
    with pytest.raises(ValueError, match="weights"):
        engine.impact_density_weighted(s, dev(engine, good).to(torch.int32), k)
    with pytest.raises(ValueError, match="weights"):
        engine.impact_density_weighted(s, dev(engine, good)[:-1], k)


def test_degenerate_clouds_are_not_solid_and_no_error(engine):
    tri = np.array([[-1.0, -1.0], [10.0, -1.0], [-1.0, 10.0]])
    t = np.linspace(0.0, 1.0, 300)

    def check(out, count, weight):
        assert out["count"] == count and not out["solid"]
        assert np.isnan(out["density"]).all() and np.isnan(out["thresholds"]).all() and out["content_w"] == [0, 0, 0]
        assert math.isnan(out["peak"]) and math.isnan(out["grid_mass"]) and out["peak_node"] == (-1, -1)
        assert math.isnan(out["f_min"]) and np.isnan(out["sample_density"].cpu().numpy()).all()
        assert out["zones"][0]["weight"] == weight
        assert np.array_equal(bits(out["grid_x"]), bits(np.linspace(*out["ranges"][0], 8)))

    # all the weight on points of one line: the off-line points are there, with weight zero
    x, y = 3.0 + 4.0 * t, 1.0 + 2.0 * t
    y[::3] += 5.0
    W = np.random.default_rng(2).integers(1, 1 << 30, 300).astype(np.int64)
    W[::3] = 0
    summ, mask, at = summary_of(x, y, True, seed=1)
    wrow = weight_row(W, at, summ.shape[1])
    keep = W > 0
    want = R.zone_weight(tri, x[keep], y[keep], W[keep])
    out = engine.impact_density_weighted(dev(engine, summ), dev(engine, wrow), dev(engine, mask), nodes=(8, 6), zones=[tri],
                                         sample_density=True)
    check(out, 200, want)
    assert out["n_zero"] == 100 and 0 < want < int(W.sum()) and out["sum_w"] == int(W.sum())
    assert out["ranges"] == ((float(x[keep].min()), float(x[keep].max())), (float(y[keep].min()), float(y[keep].max())))
    # every weight zero, and every sample masked
    for wr, mk in ((np.zeros_like(wrow), mask), (wrow, np.ones(summ.shape[1], dtype=np.uint8))):
        out = engine.impact_density_weighted(dev(engine, summ), dev(engine, wr), dev(engine, mk), nodes=(8, 6), zones=[tri],
                                             sample_density=True)
        check(out, 0, 0)
        assert out["ranges"] == ((0.0, 1.0), (0.0, 1.0)) and math.isnan(out["mean"][0]) and math.isnan(out["ess"])
        assert (out["sum_w"], out["max_w"]) == (0, 0)
    # Scott's rule with two points ... which a bandwidth matrix makes solid
    summ, mask, at = summary_of(np.array([1.0, 2.0]), np.array([0.5, 4.0]), False)
    two = dev(engine, np.array([3, 5], dtype=np.int64))
    out = engine.impact_density_weighted(dev(engine, summ), two, None, nodes=(8, 6), zones=[tri], sample_density=True)
    check(out, 2, 8)
    assert np.allclose(out["covariance"], np.cov([1.0, 2.0], [0.5, 4.0], aweights=[3, 5]), rtol=1e-14)
    assert engine.impact_density_weighted(dev(engine, summ), two, None, nodes=(8, 6), bandwidth=[[1.0, 0.0], [0.0, 1.0]])["solid"]


# ------------------------------------------------------------------------------------------------ one flown case
# tests/test_gpu_reweight.py's flight test, restated: its three-row target law
TARGET = {"mass_uncertainty": 0.01, "wind_speed_range": [3.0, 5.0], "wind_direction_range": [math.pi / 2, 3 * math.pi / 2]}


def test_a_flown_run_under_the_target_law(tmp_path, monkeypatch):
    """Planar, 4096 flights, design='random', seed 2024; a bandwidth matrix, because planar landings lie on a line.  With the
    zone a rectangle its weight is, exactly, the exceed_w of an erpl_mc_reweight call whose `extra` is the 0 / 1 indicator of
    the same rectangle; its probability lies within 5 sqrt(se_rw^2 + se_direct^2) of a run flown under the target table (the
    bound of that flight test).  The unweighted figure is printed beside it, not asserted."""
    from erpl_monte_carlo_sim_amd import plots
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer, shared_engine
    make = lambda: MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)   # noqa: E731
    mc = make()
    flown = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, seed=2024, planar=True, design="random")
    direct_mc = make()
    direct_mc.uncertainty_params.update(TARGET)
    direct = direct_mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, seed=777, planar=True, design="random")
    eng = shared_engine(mc.device)
    summ = flown["summary"]
    why = analysis._filter(summ, flown["status"], eng)[2]
    xy = summ[[RX, RY]].cpu().numpy()
    ok = (why.cpu().numpy() == 0) & np.isfinite(xy[0]) & np.isfinite(xy[1])
    # the far third of the flown landings along x, the whole line across
    x0, x1 = float(np.quantile(xy[0][ok], 2 / 3)), float(xy[0][ok].max() + 1.0)
    y0, y1 = float(xy[1][ok].min() - 10.0), float(xy[1][ok].max() + 10.0)
    rect = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
    sx = float(xy[0][ok].std())
    Hm = [[(0.2 * sx) ** 2, 0.0], [0.0, 25.0]]
    out = mc.reweighted_impact(flown, uncertainty=TARGET, zones=[rect], bandwidth=Hm, nodes=(64, 16), planar=True)
    assert out["primitive_rows"] == [12, 317, 318] and out["solid"] and out["warnings"] == []
    zone = out["zones"][0]
    # exact: the same weight through erpl_mc_reweight on the indicator of the rectangle
    _, _, factors, kinds, law, _, _ = mc._law_change_factors(flown, TARGET, None, None, True)
    ind = R.crossing(rect[:, 0], rect[:, 1], xy[0], xy[1]).astype(np.float64)
    rw = eng.reweight(factors, kinds, law, summ, mask=why, rows=["extra"], extra=torch.from_numpy(ind).to(eng.device),
                      thresholds={"extra": [0.5]}, quantiles=())
    row = rw["rows"][_abi.RW_ROW_EXTRA]
    # the map counts the samples that have an impact point and a weight; here every kept sample has the point, so the
    # populations are one (what lies outside the target's support has weight zero there and is counted as n_zero here)
    assert out["n_non_finite"] == 0 and out["count"] == rw["count"] - rw["n_zero"]
    assert out["n_zero"] == rw["n_zero"] + rw["n_outside"] and out["sum_w"] == rw["sum_w"] and out["max_w"] == rw["max_w"]
    assert zone["weight"] == row["exceed_w"][0] and 0 < zone["weight"] < out["sum_w"]
    assert abs(zone["probability"] - row["p"][0]) <= 1e-15 and abs(zone["se"] - row["p_se"][0]) <= 1e-12 * row["p_se"][0]
    assert abs(out["ess"] - rw["ess"]) <= 1e-12 * rw["ess"]
    # within the flight test's bound of a run flown under the target law
    d_why = analysis._filter(direct["summary"], direct["status"], eng)[2].cpu().numpy()
    dxy = direct["summary"][[RX, RY]].cpu().numpy()
    d_ok = (d_why == 0) & np.isfinite(dxy[0]) & np.isfinite(dxy[1])
    p_direct = float(R.crossing(rect[:, 0], rect[:, 1], dxy[0][d_ok], dxy[1][d_ok]).sum()) / int(d_ok.sum())
    se_direct = math.sqrt(p_direct * (1.0 - p_direct) / int(d_ok.sum()))
    p_flown = float(ind[ok].sum()) / int(ok.sum())
    bound = 5.0 * math.sqrt(zone["se"] ** 2 + se_direct ** 2)
    print(f"zone probability: reweighted {zone['probability']:.6g} +- {zone['se']:.3g}, direct {p_direct:.6g} +- {se_direct:.3g}, "
          f"unweighted {p_flown:.6g}; bound {bound:.3g}; ess {out['ess']:.1f} of {out['count']}; cep {out['cep']['quantiles']}")
    assert abs(zone["probability"] - p_direct) <= bound
    for p, c in zip(out["levels"], out["content_w"]):
        assert c >= p * out["sum_w"]
    assert out["thresholds"][0] >= out["thresholds"][1] >= out["thresholds"][2] > 0.0
    # the picture and the numbers
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(plots, "DPI", 60)
    out_dir = mc.plot_reweighted_impact(out)
    import json
    import os
    assert os.path.getsize(os.path.join(out_dir, "monte_carlo_reweighted_impact.png")) > 0
    saved = json.load(open(os.path.join(out_dir, "reweighted_impact.json")))
    assert saved["sum_w"] == out["sum_w"] and saved["zones"][0]["weight"] == zone["weight"] and saved["thresholds"] == out["thresholds"]
