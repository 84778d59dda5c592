"""erpl_mc_impact_density on the device: the kernel density at the nodes and at the samples against an extended-precision
sum, the rule against scipy.stats.gaussian_kde, and what has to hold exactly - the nodes, the count, the order statistics
behind the thresholds, the zone counts, the peak - plus the summation-order contract, the degenerate clouds and a real run.

The density tolerance is MEASURED, not fixed.  Truth is the direct quadratic form in np.longdouble (63-bit mantissa) with the
H the call returned.  Two float64 NumPy formulations are compared against it - the direct quadratic form, and the
Cholesky-whitened sum as scipy.stats.gaussian_kde does it - and nodes fall into three classes by truth / peak: body >= 1e-12,
tail [1e-280, 1e-12), dead < 1e-280.  In body and tail the device's worst relative error may be at most 4 x the worse of the
two formulations' errors in that class (explicit FMAs, another operation order, a device exp within 2 ulp) plus
(m + 64) * 2^-53 (the device's sequential sum, which NumPy's pairwise sum does not have); dead nodes must be <= 1e-279 x peak.
Every case prints its figures (pytest -s)."""
import math

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models, sampling

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
    """(summary [16, n], mask [n] or None, the indices of the counted samples): with junk the m points are interleaved, in
    their order, with masked samples and with NaN / +-inf entries in either row."""
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


def dev(engine, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def truth_ld(qx, qy, px, py, Hm):
    """sum_i exp(-(q - p_i)' H^-1 (q - p_i) / 2) / (m 2 pi sqrt(det H)) in long double, for the query points q."""
    hxx, hxy, hyy = LD(Hm[0][0]), LD(Hm[0][1]), LD(Hm[1][1])
    det = hxx * hyy - hxy * hxy
    a, b, c = hyy / det, -hxy / det, hxx / det
    qx, qy, px, py = (np.asarray(v, dtype=np.float64).astype(LD) for v in (qx, qy, px, py))
    out = np.zeros(len(qx), dtype=LD)
    step = max(1, 2_000_000 // max(len(qx), 1))
    for s in range(0, len(px), step):
        dx, dy = qx[:, None] - px[None, s:s + step], qy[:, None] - py[None, s:s + step]
        out += np.exp(LD(-0.5) * (a * dx * dx + LD(2) * b * dx * dy + c * dy * dy)).sum(axis=1)
    return out / (LD(len(px)) * LD(2) * LD(np.pi) * np.sqrt(det))


def direct_f64(qx, qy, px, py, Hm):
    hxx, hxy, hyy = Hm[0][0], Hm[0][1], Hm[1][1]
    det = hxx * hyy - hxy * hxy
    a, b, c = hyy / det, -hxy / det, hxx / det
    out = np.zeros(len(qx))
    step = max(1, 2_000_000 // max(len(qx), 1))
    for s in range(0, len(px), step):
        dx, dy = qx[:, None] - px[None, s:s + step], qy[:, None] - py[None, s:s + step]
        out += np.exp(-0.5 * (a * dx * dx + 2.0 * b * dx * dy + c * dy * dy)).sum(axis=1)
    return out / (len(px) * 2.0 * np.pi * np.sqrt(det))


def whitened_f64(qx, qy, px, py, Hm):
    """scipy.stats.gaussian_kde's evaluation: both sets through the inverse Cholesky factor, then squared distances."""
    L = np.linalg.cholesky(np.asarray(Hm, dtype=np.float64))
    W = np.linalg.inv(L)
    P, Q = W @ np.vstack([px, py]), W @ np.vstack([qx, qy])
    out = np.zeros(len(qx))
    step = max(1, 2_000_000 // max(len(qx), 1))
    for s in range(0, len(px), step):
        du, dv = Q[0][:, None] - P[0][None, s:s + step], Q[1][:, None] - P[1][None, s:s + step]
        out += np.exp(-0.5 * (du * du + dv * dv)).sum(axis=1)
    return out / (len(px) * 2.0 * np.pi * L[0, 0] * L[1, 1])


def judge(label, got, qx, qy, px, py, Hm):
    """The measured-tolerance comparison of the module docstring for the device values `got` at the query points."""
    assert np.finfo(LD).nmant == 63   # x86-64 extended precision: a long double that is a double would be no truth
    m = len(px)
    t = truth_ld(qx, qy, px, py, Hm)
    refs = [direct_f64(qx, qy, px, py, Hm), whitened_f64(qx, qy, px, py, Hm)]
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
        print(f"{label} {name}: {int(sel.sum())} nodes, device {e_dev:.3g}, direct {e_ref[0]:.3g}, whitened {e_ref[1]:.3g}, "
              f"bound {bound:.3g}")
        assert e_dev <= bound, (label, name, e_dev, e_ref, bound)


def wide_ranges(x, y):
    """Ranges 1.5 spans beyond the cloud: body, tail and (for the larger clouds, whose bandwidth is small) dead nodes."""
    sx, sy = x.max() - x.min(), y.max() - y.min()
    return (x.min() - 1.5 * sx, x.max() + 1.5 * sx), (y.min() - 1.5 * sy, y.max() + 1.5 * sy)


# (label, cloud, m, nodes, interleaved with masked / non-finite samples)
CASES = [("m3", "mix", 3, (64, 48), False), ("m63", "gauss", 63, (64, 48), True), ("m64", "mix", 64, (64, 48), True),
         ("m65", "gauss", 65, (64, 48), False), ("m255", "mix", 255, (64, 48), True), ("m256", "gauss", 256, (64, 48), True),
         ("m257", "mix", 257, (64, 48), True), ("m1025", "gauss", 1025, (64, 48), True),
         ("m4099-gauss", "gauss", 4099, (64, 48), True), ("m4099-mix", "mix", 4099, (64, 48), False),
         ("3x5", "gauss", 257, (3, 5), True), ("255x257", "gauss", 257, (255, 257), False),
         ("512x512", "mix", 65, (512, 512), True), ("2x2", "mix", 20011, (2, 2), True)]


@pytest.mark.parametrize("label,kind,m,nodes,junk", CASES, ids=[c[0] for c in CASES])
def test_density_at_the_nodes_and_at_the_samples(engine, label, kind, m, nodes, junk):
    x, y = cloud(kind, m, 1000 + m)
    summ, mask, at = summary_of(x, y, junk, seed=m)
    ranges = wide_ranges(x, y)
    out = engine.impact_density(dev(engine, summ), dev(engine, mask), nodes=nodes, ranges=ranges, sample_density=True)
    assert out["count"] == m and out["solid"]
    Hm = out["bandwidth_matrix"]
    S = np.cov(x, y)
    scott = m ** (-1.0 / 3.0) * S   # H = (m^(-1/6))^2 S
    for got, want in ((Hm[0][0], scott[0, 0]), (Hm[0][1], scott[0, 1]), (Hm[1][1], scott[1, 1])):
        assert abs(got - want) <= 1e-12 * abs(want)
    # exact: the nodes are np.linspace of the returned range, which is the explicit one
    assert out["ranges"] == (tuple(float(v) for v in ranges[0]), tuple(float(v) for v in ranges[1]))
    assert np.array_equal(bits(out["grid_x"]), bits(np.linspace(*out["ranges"][0], nodes[0])))
    assert np.array_equal(bits(out["grid_y"]), bits(np.linspace(*out["ranges"][1], nodes[1])))
    gx, gy = np.meshgrid(out["grid_x"], out["grid_y"], indexing="ij")   # x-major
    dens = out["density"]
    assert dens.shape == nodes
    judge(label + " grid", dens.ravel(), gx.ravel(), gy.ravel(), x, y, Hm)
    # exact: the peak and its node, and the mass to 1e-12
    assert out["peak"] == dens.max() and out["peak_node"] == tuple(int(v) for v in np.unravel_index(np.argmax(dens), nodes))
    cell = ((ranges[0][1] - ranges[0][0]) / (nodes[0] - 1)) * ((ranges[1][1] - ranges[1][0]) / (nodes[1] - 1))
    assert abs(out["grid_mass"] - dens.sum() * cell) <= 1e-12 * dens.sum() * cell
    # the samples: NaN exactly where a sample is not counted; every counted one against the truth (at 20 011 points, where
    # all pairs in long double would take minutes, every 39th)
    row = out["sample_density"].cpu().numpy()
    counted = np.zeros(summ.shape[1], dtype=bool)
    counted[at] = True
    assert np.isnan(row[~counted]).all() and np.isfinite(row[counted]).all()
    pick = np.arange(m) if m <= 4099 else np.arange(0, m, m // 512)
    judge(label + " samples", row[at][pick], x[pick], y[pick], x, y, Hm)
    # exact: the order statistics behind every threshold are those of the device's own row
    s = np.sort(row[counted])
    st = out["sample_density_stats"]
    assert st["count"] == m and st["min"] == s[0] and st["max"] == s[-1]
    for k, p in enumerate(out["levels"]):
        pos = (1.0 - p) * (m - 1)
        lo = int(math.floor(pos))
        hi = min(lo + 1, m - 1)
        assert st["order_lo"][k] == s[lo] and st["order_hi"][k] == s[hi], (k, p)
        assert out["thresholds"][k] == s[lo] + (s[hi] - s[lo]) * (pos - lo)
        inside = int((row[counted] >= out["thresholds"][k]).sum())
        assert abs(inside / m - p) <= 1.0 / m + 1e-12, (p, inside)


def test_many_sources_per_slice_on_a_stride_of_the_nodes(engine):
    """20 011 sources under 65 535 queries: slices of two LDS tiles each (erpl_dens_slices).  All nodes in long double would
    take minutes, so every 127th node is judged; the others are held to the float64 neighbours' smoothness only through
    the peak and the mass of the full grid."""
    m, nodes = 20011, (255, 257)
    x, y = cloud("gauss", m, 5)
    summ, mask, at = summary_of(x, y, True, seed=5)
    out = engine.impact_density(dev(engine, summ), dev(engine, mask), nodes=nodes, levels=())
    assert out["count"] == m and out["solid"] and out["thresholds"] == []
    gx, gy = np.meshgrid(out["grid_x"], out["grid_y"], indexing="ij")
    pick = np.arange(0, nodes[0] * nodes[1], 127)
    judge("m20011 255x257", out["density"].ravel()[pick], gx.ravel()[pick], gy.ravel()[pick], x, y, out["bandwidth_matrix"])
    assert out["peak"] == out["density"].max() and 0.98 < out["grid_mass"] < 1.0 + 1e-6


def test_one_point_with_a_bandwidth_matrix(engine):
    Hm = [[4.0, 1.5], [1.5, 2.25]]
    summ = np.zeros((_abi.SUMMARY_DIM, 3))
    summ[RX], summ[RY] = [7.0, 10.5, np.nan], [1.0, -2.25, 0.0]
    mask = np.array([3, 0, 0], dtype=np.uint8)
    out = engine.impact_density(dev(engine, summ), dev(engine, mask), nodes=(9, 7), bandwidth=Hm, sample_density=True)
    assert out["count"] == 1 and out["solid"] and out["bandwidth_matrix"] == Hm and out["mean"] == [10.5, -2.25]
    assert np.isnan(out["covariance"][0][0])   # no sample covariance of one point
    assert out["ranges"] == ((10.5 - 3 * 2.0, 10.5 + 3 * 2.0), (-2.25 - 3 * 1.5, -2.25 + 3 * 1.5))   # pad 3 standard deviations
    gx, gy = np.meshgrid(out["grid_x"], out["grid_y"], indexing="ij")
    judge("m1 matrix", out["density"].ravel(), gx.ravel(), gy.ravel(), np.array([10.5]), np.array([-2.25]), Hm)
    row = out["sample_density"].cpu().numpy()
    norm = 1.0 / (2.0 * np.pi * math.sqrt(4.0 * 2.25 - 2.25))
    assert np.isnan(row[[0, 2]]).all() and abs(row[1] - norm) <= 4 * U * norm and abs(out["norm"] - norm) <= 4 * U * norm
    assert out["thresholds"] == [row[1]] * 3
    assert out["peak_node"] == (4, 3) and out["peak"] == out["density"][4, 3]


def test_the_rule_is_scipys(engine):
    """Pins the definition, not the rounding: Scott's rule on the sample covariance, the density and the density at the
    samples against scipy.stats.gaussian_kde on body nodes to 1e-9."""
    stats = pytest.importorskip("scipy.stats")
    for kind, m, scale in (("gauss", 500, 1.0), ("mix", 333, 0.7)):
        x, y = cloud(kind, m, 31)
        summ, mask, at = summary_of(x, y, True, seed=31)
        out = engine.impact_density(dev(engine, summ), dev(engine, mask), nodes=(40, 30), bandwidth=None if scale == 1.0 else scale,
                                    sample_density=True)
        kde = stats.gaussian_kde(np.vstack([x, y]), bw_method=None if scale == 1.0 else m ** (-1.0 / 6.0) * scale)
        assert np.allclose(np.asarray(out["bandwidth_matrix"]), kde.covariance, rtol=1e-12, atol=0.0)
        # the automatic range: min / max -+ pad bandwidth standard deviations
        want = ((x.min() - 3.0 * math.sqrt(kde.covariance[0, 0]), x.max() + 3.0 * math.sqrt(kde.covariance[0, 0])),
                (y.min() - 3.0 * math.sqrt(kde.covariance[1, 1]), y.max() + 3.0 * math.sqrt(kde.covariance[1, 1])))
        assert np.allclose(np.asarray(out["ranges"]), np.asarray(want), rtol=1e-12, atol=0.0)
        gx, gy = np.meshgrid(out["grid_x"], out["grid_y"], indexing="ij")
        ref = kde(np.vstack([gx.ravel(), gy.ravel()])).reshape(40, 30)
        body = ref >= 1e-12 * ref.max()
        assert body.sum() > 300 and np.abs(out["density"][body] / ref[body] - 1.0).max() <= 1e-9
        own = kde(kde.dataset)   # own term included
        assert np.abs(out["sample_density"].cpu().numpy()[at] / own - 1.0).max() <= 1e-9


def crossing(vx, vy, x, y):
    """The even-odd rule of include/erpl_mc.h in NumPy, every operation rounded on its own."""
    inside = np.zeros(len(x), dtype=bool)
    nv = len(vx)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(nv):
            j = i - 1 if i else nv - 1
            straddles = (vy[i] > y) != (vy[j] > y)
            left = x < (vx[j] - vx[i]) * (y - vy[i]) / (vy[j] - vy[i]) + vx[i]
            inside ^= straddles & left
    return inside


def test_zone_counts_are_numpys_to_the_last_sample(engine):
    x, y = cloud("mix", 6000, 9)
    hexagon = np.array([[-700.0, -110.0], [-100.0, -90.0], [-80.0, 600.0], [-300.0, 620.0], [-310.0, 100.0], [-690.0, 120.0]])
    probe = crossing(hexagon[:, 0], hexagon[:, 1], np.array([-500.0, -500.0, -200.0]), np.array([400.0, 0.0, 400.0]))
    assert list(probe) == [False, True, True]   # an L: the first point lies in its notch
    empty = np.array([[5000.0, 5000.0], [5100.0, 5000.0], [5000.0, 5200.0]])
    box = np.array([[-1e4, -1e4], [1e4, -1e4], [1e4, 1e4], [-1e4, 1e4]])
    sliver = np.array([[-400.0, 250.0], [700.0, -300.0], [700.0, -299.0]])   # between the clusters, nearly degenerate
    # samples exactly on a vertex of the hexagon, on its horizontal-free edges' ends and on the horizontal edges of the box
    x[:6], y[:6] = hexagon[:, 0], hexagon[:, 1]
    x[6:9], y[6:9] = [0.0, -1e4, 1e4], [-1e4, 1e4, 1e4]   # on the lower edge, on two upper vertices of the box
    x[9], y[9] = 1e4, 0.0                                   # on the right edge
    summ, mask, at = summary_of(x, y, True, seed=9)
    zones = [hexagon, empty, box, sliver]
    out = engine.impact_density(dev(engine, summ), dev(engine, mask), nodes=(16, 16), levels=(), zones=zones)
    assert out["count"] == 6000
    want = [int(crossing(z[:, 0], z[:, 1], x, y).sum()) for z in zones]
    print("zones inside:", [z["inside"] for z in out["zones"]], "numpy:", want)
    assert [z["inside"] for z in out["zones"]] == want
    assert want[1] == 0 and want[2] >= 5990 and 0 < want[0] < 6000 and 0 < want[3] < 6000
    # through analysis.impact_probability: the probabilities and their own Wilson intervals (no status: nothing but the
    # bounds of the filter, which these rows of zeros fail - so filter on rows that pass)
    summ[_abi.SUM_APOGEE_ALT], summ[_abi.SUM_RANGE], summ[_abi.SUM_FLIGHT_TIME] = 3000.0, 500.0, 60.0
    res = analysis.impact_probability(dev(engine, summ), engine=engine, nodes=(16, 16), levels=(), zones=zones)
    assert res["count"] == int((np.isfinite(summ[RX]) & np.isfinite(summ[RY])).sum())   # the mask is the filter's now
    for z in res["zones"]:
        assert z["probability"] == z["inside"] / res["count"]
        assert z["interval"] == analysis.wilson_interval(z["inside"], res["count"]) and z["interval"][0] <= z["probability"] <= z["interval"][1]


def test_same_bytes_twice_and_for_the_dense_population(engine):
    x, y = cloud("mix", 4099, 3)
    summ, mask, at = summary_of(x, y, True, seed=3)
    zones = [np.array([[-600.0, 0.0], [-200.0, 0.0], [-400.0, 500.0]])]
    kw = dict(nodes=(64, 48), zones=zones, sample_density=True)
    a = engine.impact_density(dev(engine, summ), dev(engine, mask), **kw)
    b = engine.impact_density(dev(engine, summ), dev(engine, mask), **kw)
    dense, _, _ = summary_of(x, y, False)
    c = engine.impact_density(dev(engine, dense), None, **kw)
    for other in (b, c):
        assert np.array_equal(bits(a["density"]), bits(other["density"]))
        assert np.array_equal(bits(a["thresholds"]), bits(other["thresholds"]))
        assert np.array_equal(bits(a["grid_x"]), bits(other["grid_x"])) and np.array_equal(bits(a["grid_y"]), bits(other["grid_y"]))
        assert a["bandwidth_matrix"] == other["bandwidth_matrix"] and a["mean"] == other["mean"]
        assert (a["peak"], a["peak_node"], a["grid_mass"]) == (other["peak"], other["peak_node"], other["grid_mass"])
        assert a["zones"][0]["inside"] == other["zones"][0]["inside"]
    assert np.array_equal(a["sample_density"].cpu().numpy().view(np.int64), b["sample_density"].cpu().numpy().view(np.int64))
    assert np.array_equal(bits(a["sample_density"].cpu().numpy()[at]), bits(c["sample_density"].cpu().numpy()))


def test_degenerate_clouds_are_not_solid_and_no_error(engine):
    tri = np.array([[-1.0, -1.0], [10.0, -1.0], [-1.0, 10.0]])
    t = np.linspace(0.0, 1.0, 300)

    def check(out, count, inside):
        assert out["count"] == count and not out["solid"]
        assert np.isnan(out["density"]).all() and np.isnan(out["thresholds"]).all()
        assert math.isnan(out["peak"]) and math.isnan(out["grid_mass"]) and out["peak_node"] == (-1, -1)
        assert out["sample_density_stats"]["count"] == 0 and np.isnan(out["sample_density"].cpu().numpy()).all()
        assert out["zones"][0]["inside"] == inside
        assert np.array_equal(bits(out["grid_x"]), bits(np.linspace(*out["ranges"][0], 8)))

    # all counted samples on one line
    x, y = 3.0 + 4.0 * t, 1.0 + 2.0 * t
    summ, mask, at = summary_of(x, y, True, seed=1)
    want = int(crossing(tri[:, 0], tri[:, 1], x, y).sum())
    out = engine.impact_density(dev(engine, summ), dev(engine, mask), nodes=(8, 6), zones=[tri], sample_density=True)
    check(out, 300, want)
    assert 0 < want < 300 and out["ranges"] == ((3.0, 7.0), (1.0, 3.0))
    # every sample masked
    out = engine.impact_density(dev(engine, summ), dev(engine, np.ones(summ.shape[1], dtype=np.uint8)), nodes=(8, 6),
                                zones=[tri], sample_density=True)
    check(out, 0, 0)
    assert out["ranges"] == ((0.0, 1.0), (0.0, 1.0)) and math.isnan(out["mean"][0])
    # Scott's rule with two points
    summ, mask, at = summary_of(np.array([1.0, 2.0]), np.array([0.5, 4.0]), False)
    out = engine.impact_density(dev(engine, summ), None, nodes=(8, 6), zones=[tri], sample_density=True)
    check(out, 2, 2)
    assert np.allclose(out["covariance"], np.cov([1.0, 2.0], [0.5, 4.0]), rtol=1e-15)
    # ... which a bandwidth matrix makes solid
    assert engine.impact_density(dev(engine, summ), None, nodes=(8, 6), bandwidth=[[1.0, 0.0], [0.0, 1.0]])["solid"]


def test_impact_probability_of_a_real_run(engine, tmp_path, monkeypatch):
    from erpl_monte_carlo_sim_amd import plots
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    db = sampling.synthetic_dispersions(4096, models.Rocket(), H.make_motor("liquid"), models.WindModel(), H.EXAMPLE_IC,
                                        engine.device, precision=_abi.PREC_F64_FAST, seed=2024, engine=engine)
    summ, status = engine.run(db)
    torch.cuda.synchronize()
    keep = analysis.native_statistics(summ, status, engine=engine)["valid_mask"].cpu().numpy()
    xy = summ[[RX, RY]].cpu().numpy()
    counted = keep & np.isfinite(xy[0]) & np.isfinite(xy[1])
    cx, cy = np.median(xy[0][counted]), np.median(xy[1][counted])
    sx, sy = xy[0][counted].std(), xy[1][counted].std()
    zones = [np.array([[cx - sx, cy - sy], [cx + sx, cy - sy], [cx + sx, cy + sy], [cx - sx, cy + sy]]),
             np.array([[cx + 50 * sx, cy], [cx + 51 * sx, cy], [cx + 50 * sx, cy + sy]])]
    res = analysis.impact_probability(summ, status, engine=engine, zones=zones, sample_density=True)
    m = res["count"]
    assert m == int(counted.sum()) and m <= res["n_samples"] and res["solid"] and m >= 3   # Set S keeps a few per cent of its samples
    row = res["sample_density"].cpu().numpy()
    assert np.array_equal(np.isfinite(row), counted)
    for p, t in zip(res["levels"], res["thresholds"]):
        assert abs(int((row[counted] >= t).sum()) / m - p) <= 1.0 / m + 1e-12
    assert res["thresholds"][0] > res["thresholds"][1] > res["thresholds"][2] > 0.0
    for z, poly in zip(res["zones"], zones):
        assert z["inside"] == int(crossing(poly[:, 0], poly[:, 1], xy[0][counted], xy[1][counted]).sum())
        assert z["interval"][0] <= z["probability"] <= z["interval"][1] and z["probability"] == z["inside"] / m
    assert 0 < res["zones"][0]["inside"] <= m and res["zones"][1]["inside"] == 0
    assert 0.5 < res["grid_mass"] < 1.5   # a Riemann sum on 128 x 128 nodes over a heavy-tailed cloud
    # the picture and the numbers, from the device dict and from records
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(plots, "DPI", 60)
    mc = MonteCarloAnalyzer(models.Rocket(), H.make_motor("liquid"), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    out_dir = mc.plot_impact_probability({"summary": summ, "status": status}, zones=zones)
    import json
    import os
    assert os.path.getsize(os.path.join(out_dir, "monte_carlo_impact_probability.png")) > 0
    saved = json.load(open(os.path.join(out_dir, "impact_probability.json")))
    assert saved["count"] == m and saved["thresholds"] == res["thresholds"] and "sample_density" not in saved
    assert saved["zones"][0]["inside"] == res["zones"][0]["inside"]
    records = [{"apogee_altitude": 3000.0, "range": 100.0, "flight_time": 50.0, "impact_position": [float(a), float(b), 0.0]}
               for a, b in zip(xy[0][counted], xy[1][counted])]
    again = mc.impact_probability({"results": records}, nodes=(32, 32))
    assert again["count"] == m and again["solid"] and again["density"].shape == (32, 32)
