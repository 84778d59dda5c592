"""erpl_mc_histogram / erpl_mc_histogram_xy / erpl_mc_dispersion on the device against NumPy on host copies of the same
tensors.

Histograms - exact, no tolerance: every count, counted / below / above / outside, and every edge BITWISE against
np.histogram / np.histogram2d of the finite values whose mask byte is 0.

Dispersion - exact: count, min / max of the miss distance and every order_lo / order_hi against np.sort of NumPy's
sqrt(dx*dx + dy*dy).  (Should the device square root differ from NumPy's in the last bit on some value, `check_miss`
compares the device's miss row to NumPy's within one ulp - np.spacing - and takes the order statistics against the
device's own row; it prints which of the two it did.)  Rounded quantities at the 1e-12 bar of test_gpu_analysis.py,
scaled the same way: means by mean |x|, covariances by sqrt(cxx cyy), both eigenvalues by var_major, quantiles by
max(|order_lo|, |order_hi|).  inside[p] must lie between NumPy's counts of d2 <= k2 (1 - 1e-9) and d2 <= k2 (1 + 1e-9),
a band for rounding only: the clouds are drawn from continuous distributions with correlation <= 0.9, where the band
holds 10^6 * 1e-9 * k2 * exp(-k2 / 2) / 2 < 1e-3 samples in expectation; the test prints how many fall inside it and
fails if more than 2 do."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models, plots, sampling

import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-12
BINS = [1, 2, 7, 50, 256, 1024]
DEFAULT_ROWS = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
CONST_ROW = 3


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def counted_values(summ, mask, row, partner=None):
    keep = np.isfinite(summ[row]) if mask is None else (mask == 0) & np.isfinite(summ[row])
    if partner is not None:
        keep &= np.isfinite(summ[partner])
    return summ[row][keep]


def upload(engine, summ, mask):
    ds = torch.from_numpy(np.ascontiguousarray(summ)).to(engine.device)
    dm = None if mask is None else torch.from_numpy(mask).to(engine.device)
    return ds, dm


def check_hist(engine, ds, dm, summ, mask, rows, bins, ranges=None):
    """One erpl_mc_histogram call against np.histogram row by row."""
    edges, counts, info = engine.histogram(ds, dm, rows=rows, bins=bins, ranges=ranges)
    blist = [bins] * len(rows) if np.isscalar(bins) else list(bins)
    for j, r in enumerate(rows):
        x = counted_values(summ, mask, r)
        rg = None if ranges is None else ranges[j]
        ref_counts, ref_edges = np.histogram(x, blist[j], range=rg)
        assert np.array_equal(bits(edges[j]), bits(ref_edges)), (r, blist[j], rg)
        assert counts[j].dtype == np.int64 and np.array_equal(counts[j], ref_counts), (r, blist[j], rg)
        assert info["counted"][j] == len(x), r
        lo, hi = ref_edges[0], ref_edges[-1]
        assert info["below"][j] == int((x < lo).sum()) and info["above"][j] == int((x > hi).sum()), r
        assert info["counted"][j] == counts[j].sum() + info["below"][j] + info["above"][j]
        assert info["lo"][j] == lo and info["hi"][j] == hi, r
    return edges, counts, info


def check_hist2d(engine, ds, dm, summ, mask, row_x, row_y, bins, ranges=None):
    counts, ex, ey, info = engine.histogram2d(ds, dm, row_x, row_y, bins=bins, ranges=ranges)
    x, y = counted_values(summ, mask, row_x, row_y), counted_values(summ, mask, row_y, row_x)
    if ranges is not None and (ranges[0] is None or ranges[1] is None):     # np.histogram2d takes all of `range` or none
        full = [(x.min(), x.max()) if len(x) else (0.0, 1.0), (y.min(), y.max()) if len(y) else (0.0, 1.0)]
        rg = [full[k] if ranges[k] is None else ranges[k] for k in range(2)]
    else:
        rg = ranges
    ref, rex, rey = np.histogram2d(x, y, bins=bins, range=rg)
    assert np.array_equal(bits(ex), bits(rex)) and np.array_equal(bits(ey), bits(rey)), (row_x, row_y, bins, ranges)
    assert counts.dtype == np.int64 and np.array_equal(counts, ref.astype(np.int64)), (row_x, row_y, bins, ranges)
    assert info["counted"] == len(x) and info["outside"] == len(x) - int(ref.sum())
    assert (info["lo_x"], info["hi_x"], info["lo_y"], info["hi_y"]) == (rex[0], rex[-1], rey[0], rey[-1])
    return counts, ex, ey, info


# ------------------------------------------------------------------ 1: the reference's own picture
def golden_columns():
    g = H.load_json("stats.json")
    inp = g["inputs"]
    keep = [i for i in range(len(inp["apogee_altitude"])) if i != inp["none_index"]]
    summ = np.zeros((16, len(keep)))
    summ[_abi.SUM_APOGEE_ALT] = [inp["apogee_altitude"][i] for i in keep]
    summ[_abi.SUM_RANGE] = [inp["range"][i] for i in keep]
    summ[_abi.SUM_FLIGHT_TIME] = [inp["flight_time"][i] for i in keep]
    return g, summ


def test_golden_histograms_of_the_reference(engine):
    """axes.hist(finite_values, bins=50) of monte_carlo.py:568-592 on the inputs of tests/golden/stats.json."""
    g, summ = golden_columns()
    ds, _ = upload(engine, summ, None)
    res, why = engine.analyze(ds, reasons=True)
    mask = why.cpu().numpy()
    assert int((mask == 0).sum()) == g["n_samples"]
    check_hist(engine, ds, why, summ, mask, DEFAULT_ROWS, 50)
    check_hist2d(engine, ds, why, summ, mask, _abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, 50)
    out = analysis.native_distributions(ds, engine=engine)
    ok = ~analysis.outlier_mask(summ[_abi.SUM_APOGEE_ALT], summ[_abi.SUM_RANGE], summ[_abi.SUM_FLIGHT_TIME])
    for r in DEFAULT_ROWS:
        ref_counts, ref_edges = np.histogram(summ[r][ok], 50)
        assert np.array_equal(out[r]["counts"], ref_counts) and np.array_equal(bits(out[r]["edges"]), bits(ref_edges))
    assert out["n_samples"] == g["n_samples"] and out["n_outliers"] == g["n_outliers"]
    # without a mask every finite value counts
    check_hist(engine, ds, None, summ, None, DEFAULT_ROWS, 50)


# ------------------------------------------------------------------ 2: a million samples, every row, awkward values
def explicit_range(x):
    """An explicit range that leaves values on both sides: the 10 % and 90 % points of the counted values."""
    xs = np.sort(x)
    return float(xs[len(xs) // 10]), float(xs[(9 * len(xs)) // 10])


@pytest.fixture(scope="module")
def big(engine):
    """All 16 rows built like big_case() of test_gpu_analysis.py (non-finite values, +-0.0, a constant, 1e90 and 1e-300
    scales), a mask that drops about half of the samples, and - in every row but the constant one - every edge of every
    bin count of BINS, one ulp below it and one ulp above it, for the automatic range and for the explicit one."""
    rng = np.random.RandomState(2025)
    n = 2 ** 20 + 12345
    s = np.zeros((16, n))

    def sprinkle(x, frac=0.30):
        k = rng.random_sample(n) < frac
        x[k] = rng.choice([np.nan, np.inf, -np.inf], size=int(k.sum()))
        return x

    s[0] = rng.normal(25000, 20000, n)
    s[1] = rng.normal(0, 3000, n)
    s[2] = rng.randint(2000, 60001, n).astype(np.float64)
    s[3] = 7.0
    s[4] = sprinkle(np.abs(rng.normal(50000, 90000, n)))
    s[5] = np.round(rng.normal(300, 150, n) / 2) * 2
    s[6] = sprinkle(rng.normal(1000, 10, n))
    z = rng.choice([0.0, -0.0, 1e-300, -1e-300, 3e-300, -2.5e-300], size=n)
    s[7] = z * np.where(np.abs(z) > 0, rng.uniform(0.5, 2.0, n), 1.0)
    s[8] = rng.normal(0, 3000, n)
    s[9] = rng.uniform(-1.0, 1.0, n)
    s[10] = rng.exponential(1.0, n)
    s[11] = rng.normal(-5000, 100, n)
    s[12] = rng.normal(0, 1, n) * 1e90
    s[13] = rng.lognormal(0, 3, n)
    s[14] = np.round(rng.normal(0, 2, n))
    s[15] = rng.normal(1e-5, 1e-7, n)
    mask = rng.choice(np.array([0, 0, 1, 2, 8, 33], dtype=np.uint8), size=n)   # a third of the bytes are 0
    mask[rng.random_sample(n) < 0.25] = 0                                        # -> half of the samples count
    ranges = {}
    for r in range(16):
        x = counted_values(s, mask, r)
        ranges[r] = (7.0, 7.0) if r == CONST_ROW else explicit_range(x)
        if r == CONST_ROW:
            continue
        plants = []
        for lo, hi in ((x.min(), x.max()), ranges[r]):
            for b in BINS:
                e = np.linspace(lo, hi, b + 1)
                plants += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
        plants = np.concatenate(plants)
        plants = plants[(plants >= x.min()) & (plants <= x.max())]          # the automatic range stays what it was
        free = np.flatnonzero((mask == 0) & (s[r] != x.min()) & (s[r] != x.max()))
        s[r][rng.choice(free, size=len(plants), replace=False)] = plants
        x2 = counted_values(s, mask, r)
        assert x2.min() == x.min() and x2.max() == x.max()
    frac = float((mask != 0).mean())
    assert 0.25 < frac < 0.75
    ds, dm = upload(engine, s, mask)
    return {"summ": s, "mask": mask, "ds": ds, "dm": dm, "ranges": ranges, "n": n}


@pytest.mark.parametrize("bins", BINS)
def test_a_million_samples_all_rows_exact(engine, big, bins):
    rows = list(range(16))
    _, counts, info = check_hist(engine, big["ds"], big["dm"], big["summ"], big["mask"], rows, bins)
    assert all(b == 0 and a == 0 for b, a in zip(info["below"], info["above"]))
    assert counts[CONST_ROW].max() == info["counted"][CONST_ROW] > 0                 # 7.0 in [6.5, 7.5]: one bin holds all
    _, counts, info = check_hist(engine, big["ds"], big["dm"], big["summ"], big["mask"], rows, bins,
                                 ranges=[big["ranges"][r] for r in rows])
    assert all(info["below"][r] > 0 and info["above"][r] > 0 for r in rows if r != CONST_ROW)
    assert all(counts[r][-1] > 0 for r in rows if r != CONST_ROW)                    # x == hi is in the last bin


def test_mixed_bins_and_ranges_in_one_call_and_repeatable(engine, big):
    rows = [12, 0, 7, CONST_ROW, 4, 15, 14]
    bins = [1024, 7, 256, 2, 50, 1, 1000]
    ranges = [None, big["ranges"][0], None, (0.0, 7.0), big["ranges"][4], None, (-3.0, -3.0)]
    _, counts, info = check_hist(engine, big["ds"], big["dm"], big["summ"], big["mask"], rows, bins, ranges)
    assert counts[3][1] == info["counted"][3] and counts[3][0] == 0                  # 7.0 == hi: the last bin
    # the same inputs into zero-initialised blocks give the same bytes
    spec = _abi.ErplHistSpec()
    spec.n_rows = len(rows)
    spec.rows[:len(rows)], spec.bins[:len(rows)] = rows, bins
    for j, rg in enumerate(ranges):
        spec.lo[j], spec.hi[j] = (float("nan"), float("nan")) if rg is None else rg
    blocks = []
    for _ in range(2):
        edges = np.zeros((len(rows), _abi.HIST_MAX_BINS + 1))
        cnt = np.zeros((len(rows), _abi.HIST_MAX_BINS), dtype=np.int64)
        res = _abi.ErplHistResult()
        C.memset(C.byref(res), 0, C.sizeof(res))
        rc = engine.lib.erpl_mc_histogram(engine._ctx, C.c_void_p(big["ds"].data_ptr()), C.c_void_p(big["dm"].data_ptr()),
                                          big["n"], C.byref(spec), C.c_void_p(edges.ctypes.data), C.c_void_p(cnt.ctypes.data),
                                          C.byref(res), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        blocks.append(edges.tobytes() + cnt.tobytes() + bytes(res))
    assert blocks[0] == blocks[1]
    assert np.array_equal(cnt[1, :7], counts[1]) and not cnt[1, 7:].any()            # the rest of a line is zero


@pytest.mark.parametrize("bins", [(1, 1), (7, 50), (64, 64), (65, 64), (256, 50), (256, 256)])
def test_a_million_samples_2d_exact(engine, big, bins):
    """(64, 64) is the largest grid counted in the LDS tile, (65, 64) the smallest that goes to the global cells."""
    a = big
    for rx, ry in ((0, 4), (12, 7), (2, CONST_ROW), (6, 13)):
        check_hist2d(engine, a["ds"], a["dm"], a["summ"], a["mask"], rx, ry, bins)
        c, _, _, info = check_hist2d(engine, a["ds"], a["dm"], a["summ"], a["mask"], rx, ry, bins,
                                     ranges=(a["ranges"][rx], a["ranges"][ry]))
        assert info["outside"] > 0 and c.sum() > 0
    check_hist2d(engine, a["ds"], a["dm"], a["summ"], a["mask"], 0, 4, bins, ranges=(None, a["ranges"][4]))
    check_hist2d(engine, a["ds"], None, a["summ"], None, 9, 10, bins)


def test_2d_repeatable(engine, big):
    spec = _abi.ErplHist2dSpec(0, 4, 200, 180, float("nan"), float("nan"), *big["ranges"][4])
    blocks = []
    for _ in range(2):
        ex, ey, cnt = np.zeros(201), np.zeros(181), np.zeros(200 * 180, dtype=np.int64)
        res = _abi.ErplHist2dResult()
        C.memset(C.byref(res), 0, C.sizeof(res))
        rc = engine.lib.erpl_mc_histogram_xy(engine._ctx, C.c_void_p(big["ds"].data_ptr()), C.c_void_p(big["dm"].data_ptr()),
                                            big["n"], C.byref(spec), C.c_void_p(ex.ctypes.data), C.c_void_p(ey.ctypes.data),
                                            C.c_void_p(cnt.ctypes.data), C.byref(res),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        blocks.append(ex.tobytes() + ey.tobytes() + cnt.tobytes() + bytes(res))
    assert blocks[0] == blocks[1]


# ------------------------------------------------------------------ 3: tiny batches, nothing counted
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_tiny_batches(engine, n):
    rng = np.random.RandomState(n)
    summ = rng.normal(0, 100, (16, n))
    mask = (rng.random_sample(n) < 0.3).astype(np.uint8) * 5
    mask[0] = 0
    if n > 2:
        summ[2, 1], summ[5, 2] = np.nan, np.inf
    ds, dm = upload(engine, summ, mask)
    rows = list(range(16))
    for bins in (1, 50, 1024):
        check_hist(engine, ds, dm, summ, mask, rows, bins)
        check_hist(engine, ds, None, summ, None, rows, bins, ranges=[(-50.0, 80.0)] * 16)
    for bins in ((1, 1), (50, 50), (256, 256)):
        check_hist2d(engine, ds, dm, summ, mask, 2, 5, bins)
        check_hist2d(engine, ds, dm, summ, mask, 8, 9, bins, ranges=((-50.0, 80.0), None))
    check_dispersion(engine, ds, dm, summ, mask, 8, 9, centre=(10.0, -20.0), check_inside=n != 2,
                     expect_solid=False if n == 1 else None)
    check_dispersion(engine, ds, None, summ, None, 2, 5, centre=None, check_inside=n != 2)


def test_a_mask_that_leaves_nothing(engine):
    rng = np.random.RandomState(1)
    summ = rng.normal(0, 100, (16, 1000))
    mask = np.full(1000, 3, dtype=np.uint8)
    ds, dm = upload(engine, summ, mask)
    edges, counts, info = check_hist(engine, ds, dm, summ, mask, [0, 1], 50)
    assert info["counted"] == [0, 0] and not counts[0].any() and np.array_equal(edges[0], np.linspace(0.0, 1.0, 51))
    check_hist(engine, ds, dm, summ, mask, [0, 1], [3, 1024], ranges=[(-1.0, 1.0), None])
    counts, ex, ey, info = check_hist2d(engine, ds, dm, summ, mask, 0, 1, (10, 300 - 44))
    assert info["counted"] == 0 and not counts.any() and (ex[0], ex[-1], ey[0], ey[-1]) == (0.0, 1.0, 0.0, 1.0)
    out = engine.dispersion(ds, dm, miss=True)
    assert out["count"] == 0 and out["miss"]["count"] == 0
    doubles = out["mean"] + out["covariance"][0] + out["covariance"][1] + [out["var_major"], out["var_minor"], out["angle"]]
    doubles += out["centre"] + [out["miss"][k] for k in ("mean", "std", "min", "max")] + out["miss"]["quantiles"]
    doubles += out["miss"]["order_lo"] + out["miss"]["order_hi"]
    for e in out["ellipses"]:
        doubles += [e["k2"], e["semi_major"], e["semi_minor"]]
        assert e["inside"] == 0
    assert all(math.isnan(v) for v in doubles)
    assert bool(out["miss_distance"].isnan().all())


def test_an_automatic_range_that_overflows_is_refused(engine):
    summ = np.zeros((16, 100))
    summ[3, 0], summ[3, 1] = -1.5e308, 1.5e308
    ds, _ = upload(engine, summ, None)
    with pytest.raises(_abi.ErplError, match=r"rows\[1\] = 3"):
        engine.histogram(ds, rows=[0, 3], bins=10)
    with pytest.raises(_abi.ErplError, match="row_y = 3"):
        engine.histogram2d(ds, None, 0, 3, bins=10)
    edges, counts, info = engine.histogram(ds, rows=[0, 3], bins=10, ranges=[None, (-1.0, 1.0)])   # and goes on working
    assert counts[1].sum() == 98 and info["below"][1] == 1 and info["above"][1] == 1


# ------------------------------------------------------------------ 4: dispersion
def check_miss(x, y, keep, centre, miss_dev, m, qs):
    """The miss distance.  NumPy's r about the centre IN USE; bitwise equal on every sample -> order statistics against
    np.sort of NumPy's r.  Otherwise (a square root that differs in the last bit) every value within one ulp of NumPy's
    and the order statistics against the device's own row."""
    with np.errstate(invalid="ignore", over="ignore"):
        ex, ey = x - centre[0], y - centre[1]
        r = np.sqrt(ex * ex + ey * ey)
    assert np.isnan(miss_dev[~keep]).all() and not np.isnan(miss_dev[keep]).any()
    if np.array_equal(miss_dev[keep], r[keep]):
        ref = r[keep]
    else:
        worst = np.max(np.abs(miss_dev[keep] - r[keep]) / np.spacing(r[keep]))
        print(f"device sqrt differs from NumPy's by up to {worst} ulp: order statistics against the device's own row")
        assert worst <= 1.0
        ref = miss_dev[keep]
    rs = np.sort(ref)
    assert m["count"] == len(rs)
    assert m["min"] == rs[0] and m["max"] == rs[-1]
    assert abs(m["mean"] - ref.mean()) <= TOL * np.mean(np.abs(ref))
    assert abs(m["std"] - ref.std()) <= TOL * ref.std()
    for k, q in enumerate(qs):
        pos = q * (len(rs) - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, len(rs) - 1)
        assert m["order_lo"][k] == rs[lo] and m["order_hi"][k] == rs[hi], (q, m["order_lo"][k], rs[lo])
        assert abs(m["quantiles"][k] - np.quantile(ref, q)) <= TOL * max(abs(rs[lo]), abs(rs[hi])), q


def check_dispersion(engine, ds, dm, summ, mask, row_x, row_y, centre, levels=(0.5, 0.9, 0.99),
                     qs=(0.5, 0.9, 0.95, 0.99, 0.0, 1.0, 1.0 / 3.0), expect_solid=None, check_inside=True):
    """check_inside=False: for a cloud of two points, which lies on a line in exact arithmetic - whether rounding leaves
    det at zero is not the subject; everything else is checked all the same."""
    out = engine.dispersion(ds, dm, row_x, row_y, centre=centre, levels=levels, quantiles=qs, miss=True)
    x, y = summ[row_x], summ[row_y]
    keep = np.isfinite(x) & np.isfinite(y)
    if mask is not None:
        keep &= mask == 0
    xv, yv = x[keep], y[keep]
    assert out["count"] == len(xv) > 0
    mean = np.array([xv.mean(), yv.mean()])
    assert abs(out["mean"][0] - mean[0]) <= TOL * np.mean(np.abs(xv)) and abs(out["mean"][1] - mean[1]) <= TOL * np.mean(np.abs(yv))
    cov = np.cov(np.stack([xv, yv]), bias=True).reshape(2, 2)
    scale = math.sqrt(cov[0, 0] * cov[1, 1])
    got = np.array(out["covariance"])
    print(f"rows ({row_x}, {row_y}): count {len(xv)}, cov err {np.abs(got - cov).max() / scale if scale > 0 else 0.0:.2e} of sqrt(cxx cyy)")
    assert np.all(np.abs(got - cov) <= TOL * scale), (got, cov)
    w = np.linalg.eigh(cov)[0]
    assert abs(out["var_major"] - w[1]) <= TOL * w[1] and abs(out["var_minor"] - w[0]) <= TOL * w[1], (out["var_major"], w)
    assert abs(out["angle"] - 0.5 * math.atan2(2 * got[0, 1], got[0, 0] - got[1, 1])) <= 1e-15
    want_centre = out["mean"] if centre is None else list(centre)
    assert out["centre"] == want_centre
    det = cov[0, 0] * cov[1, 1] - cov[0, 1] ** 2
    dev_det = got[0, 0] * got[1, 1] - got[0, 1] * got[0, 1]
    solid = bool(dev_det > 0 and np.isfinite(dev_det))
    if expect_solid is not None:
        assert solid == expect_solid
    dx, dy = xv - mean[0], yv - mean[1]
    for e, p in zip(out["ellipses"], levels):
        k2 = -2.0 * math.log(1.0 - p)
        assert e["level"] == p and abs(e["k2"] - k2) <= 4e-16 * k2
        assert abs(e["semi_major"] - math.sqrt(k2 * w[1])) <= TOL * math.sqrt(k2 * w[1])
        assert abs(e["semi_minor"] - math.sqrt(k2 * max(w[0], 0.0))) <= 1e-6 * math.sqrt(k2 * w[1])   # sqrt of a difference
        if solid and w[0] > 1e-6 * w[1]:
            assert abs(e["semi_minor"] - math.sqrt(k2 * w[0])) <= 1e-9 * math.sqrt(k2 * w[0])
        if not check_inside:
            continue
        if not solid:
            assert e["inside"] == -1
            continue
        d2 = (cov[1, 1] * dx * dx - 2.0 * cov[0, 1] * dx * dy + cov[0, 0] * dy * dy) / det
        lo, hi = int((d2 <= k2 * (1 - 1e-9)).sum()), int((d2 <= k2 * (1 + 1e-9)).sum())
        print(f"  level {p}: inside {e['inside']}, NumPy {lo}..{hi}: {hi - lo} sample(s) in the rounding band")
        assert hi - lo <= 2
        assert lo <= e["inside"] <= hi
    check_miss(x, y, keep, out["centre"], out["miss_distance"].cpu().numpy(), out["miss"], qs)
    assert out["cep"] == out["miss"]["quantiles"][0]
    # the context's own row instead of the caller's: the same numbers
    again = engine.dispersion(ds, dm, row_x, row_y, centre=centre, levels=levels, quantiles=qs)
    out.pop("miss_distance")
    assert json.dumps(again, sort_keys=True) == json.dumps(out, sort_keys=True)
    return out


@pytest.fixture(scope="module")
def cloud(engine):
    """A million impact points from continuous distributions (correlation 0.8 and -0.9, a skewed pair), 30 % of one row
    non-finite, a mask that drops a third."""
    rng = np.random.RandomState(77)
    n = 10 ** 6 + 77
    s = np.zeros((16, n))
    u, v = rng.normal(0, 1, n), rng.normal(0, 1, n)
    s[8] = 1500.0 + 900.0 * u
    s[9] = -400.0 + 300.0 * (0.8 * u + 0.6 * v)
    s[0] = 25.0 * v
    s[1] = 3.0e4 - 50.0 * (0.9 * v - math.sqrt(1 - 0.81) * u)
    s[4] = rng.lognormal(3.0, 0.5, n)
    s[5] = rng.exponential(40.0, n) + 0.3 * s[4]
    k = rng.random_sample(n) < 0.3
    s[9][k] = rng.choice([np.nan, np.inf, -np.inf], size=int(k.sum()))
    mask = (rng.random_sample(n) < 1.0 / 3.0).astype(np.uint8) * 9
    ds, dm = upload(engine, s, mask)
    return {"summ": s, "mask": mask, "ds": ds, "dm": dm, "n": n}


@pytest.mark.parametrize("rows,centre", [((8, 9), (0.0, 0.0)), ((8, 9), None), ((0, 1), (3.0, 2.9e4)), ((4, 5), None)])
def test_dispersion_of_a_million_impacts(engine, cloud, rows, centre):
    out = check_dispersion(engine, cloud["ds"], cloud["dm"], cloud["summ"], cloud["mask"], rows[0], rows[1], centre,
                           levels=(0.5, 0.9, 0.99, 0.1, 0.999), expect_solid=True)
    frac = [e["inside"] / out["count"] for e in out["ellipses"]]
    if rows != (4, 5):      # Gaussian clouds hold what the level says, to sampling error
        assert all(abs(f - e["level"]) < 5e-3 for f, e in zip(frac, out["ellipses"]))
    # the major axis lies along the principal direction of NumPy's covariance
    keep = (cloud["mask"] == 0) & np.isfinite(cloud["summ"][rows[0]]) & np.isfinite(cloud["summ"][rows[1]])
    vec = np.linalg.eigh(np.cov(cloud["summ"][list(rows)][:, keep], bias=True))[1][:, 1]
    assert abs(abs(math.cos(out["angle"]) * vec[0] + math.sin(out["angle"]) * vec[1]) - 1.0) < 1e-9


def test_dispersion_without_a_mask_and_repeatable(engine, cloud):
    check_dispersion(engine, cloud["ds"], None, cloud["summ"], None, 8, 9, (0.0, 0.0), expect_solid=True)
    spec = _abi.ErplDispersionSpec()
    assert engine.lib.erpl_mc_dispersion_defaults(C.byref(spec)) == 0
    spec.centre = _abi.CENTRE_MEAN
    blocks = []
    for _ in range(2):
        res = _abi.ErplDispersion()
        C.memset(C.byref(res), 0, C.sizeof(res))
        rc = engine.lib.erpl_mc_dispersion(engine._ctx, C.c_void_p(cloud["ds"].data_ptr()), C.c_void_p(cloud["dm"].data_ptr()),
                                           cloud["n"], C.byref(spec), C.byref(res), None,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        blocks.append(bytes(res))
    assert blocks[0] == blocks[1]


def test_degenerate_clouds(engine):
    """All points on a line: det is exactly 0 (every sum below is exact), so inside is -1 and the axes are still there."""
    n = 4096
    summ = np.zeros((16, n))
    t = (np.arange(n) % 1024).astype(np.float64)
    summ[8], summ[9] = t, 2.0 * t + 1.0            # y = 2 x + 1
    summ[0], summ[1] = t, 5.0                      # a horizontal line
    summ[2], summ[3] = -3.0, 4.0                   # one point
    ds, _ = upload(engine, summ, None)
    for rx, ry in ((8, 9), (0, 1), (2, 3)):
        out = check_dispersion(engine, ds, None, summ, None, rx, ry, (0.0, 0.0), expect_solid=False)
        assert all(e["inside"] == -1 and e["semi_major"] >= 0.0 for e in out["ellipses"])
    out = engine.dispersion(ds, None, 2, 3)
    assert out["cep"] == 5.0 and out["miss"]["std"] == 0.0 and out["var_major"] == 0.0
    assert all(e["semi_major"] == 0.0 and e["semi_minor"] == 0.0 for e in out["ellipses"])
    out = engine.dispersion(ds, None, 8, 9)
    assert abs(out["angle"] - math.atan(2.0)) < 1e-12 and abs(out["var_minor"]) <= 1e-9 * out["var_major"]


# ------------------------------------------------------------------ 5: a real run and the pictures
@pytest.fixture(scope="module")
def real_run(engine):
    db = sampling.synthetic_dispersions(24000, models.Rocket(), H.make_motor("liquid"), models.WindModel(), H.EXAMPLE_IC,
                                        engine.device, precision=_abi.PREC_F64_FAST, seed=4242, engine=engine)
    summ, status = engine.run(db)
    torch.cuda.synchronize()
    return summ, status


def test_real_run_distributions_agree_with_numpy(engine, real_run):
    summ, status = real_run
    host = summ.cpu().numpy()
    ok = ~analysis.outlier_mask(host[_abi.SUM_APOGEE_ALT], host[_abi.SUM_RANGE], host[_abi.SUM_FLIGHT_TIME])
    out = analysis.native_distributions(summ, status)           # the shared engine of the tensors' device
    assert out["n_samples"] == int(ok.sum()) > 0 and np.array_equal(out["valid_mask"].cpu().numpy(), ok)
    for r in DEFAULT_ROWS:
        ref_counts, ref_edges = np.histogram(host[r][ok], 50)
        assert np.array_equal(out[r]["counts"], ref_counts) and np.array_equal(bits(out[r]["edges"]), bits(ref_edges))
        assert out[r]["counted"] == int(ok.sum())
    rows = [_abi.SUM_IMPACT_X, _abi.SUM_MAX_SPEED]
    out = analysis.native_distributions(summ, status, engine=engine, bins=[7, 1024], rows=rows)
    for r, b in zip(rows, (7, 1024)):
        x = host[r][ok]
        ref_counts, ref_edges = np.histogram(x[np.isfinite(x)], b)
        assert np.array_equal(out[r]["counts"], ref_counts) and np.array_equal(bits(out[r]["edges"]), bits(ref_edges))
    disp = analysis.landing_dispersion(summ, status, engine=engine, target=(100.0, -50.0))
    keep = ok & np.isfinite(host[_abi.SUM_IMPACT_X]) & np.isfinite(host[_abi.SUM_IMPACT_Y])
    r = np.sqrt((host[_abi.SUM_IMPACT_X][keep] - 100.0) ** 2 + (host[_abi.SUM_IMPACT_Y][keep] + 50.0) ** 2)
    assert disp["count"] == int(keep.sum()) and disp["n_samples"] == int(ok.sum()) and disp["centre"] == [100.0, -50.0]
    assert abs(disp["cep"] - np.median(r)) <= 1e-9 * np.median(r)
    print("valid", disp["n_samples"], "of 24000; CEP", disp["cep"], "ellipses", disp["ellipses"])


def test_plot_methods_on_the_device_dict(engine, real_run, tmp_path, monkeypatch, capsys):
    """The dict of run_monte_carlo_device (tensors + statistics, no per-sample results): scatter below SCATTER_MAX valid
    samples, the 2-D device histogram above; the report is written because the dict carries its numbers."""
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    monkeypatch.chdir(tmp_path)
    summ, status = real_run
    dic = analysis.device_statistics(summ, status)
    dic["summary"], dic["status"] = summ, status
    mc = MonteCarloAnalyzer(models.Rocket(), H.make_motor("liquid"), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    monkeypatch.setattr(plots, "DPI", 60)
    seen = []
    real = plots.distributions_figure
    monkeypatch.setattr(plots, "distributions_figure", lambda *a, **k: seen.append(k) or real(*a, **k))
    out_dir = mc.plot_results(dic)
    assert seen[-1]["points"] is not None and seen[-1]["density"] is None
    assert seen[-1]["points"].shape == (2, dic["n_samples"])
    monkeypatch.setattr(plots, "SCATTER_MAX", 100)
    out_dir2 = mc.plot_results(dic, save_plots=False)
    assert out_dir2 is None and seen[-1]["points"] is None
    counts, ex, ey = seen[-1]["density"]
    assert counts.shape == (plots.DENSITY_BINS, plots.DENSITY_BINS) and counts.sum() == dic["n_samples"]
    assert os.path.realpath(out_dir).startswith(os.path.realpath(str(tmp_path)))
    assert {"monte_carlo_distributions.png", "monte_carlo_report.json", "monte_carlo_report.txt",
            "simulation_results"} <= set(os.listdir(out_dir))
    text = capsys.readouterr().out
    assert f"Number of valid simulations: {dic['n_samples']}" in text and "Range Statistics:" in text
    land = mc.plot_landing_dispersion(dic, target=(0.0, 0.0))
    assert os.path.realpath(land).startswith(os.path.realpath(str(tmp_path)))
    assert {"landing_dispersion.json", "monte_carlo_landing.png"} <= set(os.listdir(land))
    saved = json.load(open(os.path.join(land, "landing_dispersion.json")))
    assert saved["count"] > 0 and saved["n_samples"] == dic["n_samples"] and len(saved["ellipses"]) == 3


def test_plot_methods_on_a_small_run_monte_carlo(engine, tmp_path, monkeypatch, capsys):
    """The last lines of the reference's example.py: 50 samples, CSV wind, plot_results and plot_trajectory_cloud_3d."""
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    monkeypatch.chdir(tmp_path)
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    mc.base_altitude_profile, mc.base_wind_profile = H.CSV_ALT, H.CSV_WIND
    res = mc.run_monte_carlo(dict(H.EXAMPLE_IC), n_samples=50)
    out_dir = mc.plot_results(res)
    text = capsys.readouterr().out
    assert f"Plots saved to: {os.path.join(out_dir, 'monte_carlo_distributions.png')}" in text
    assert f"Report saved to: {out_dir}" in text and "Monte Carlo Analysis Results:" in text
    assert f"Number of valid simulations: {res['n_samples']}" in text and f"Number of outlier simulations: {res['n_outliers']}" in text
    assert f"  Mean: {res['apogee_altitude']['mean']:.1f} m" in text
    assert {"monte_carlo_distributions.png", "monte_carlo_report.json", "monte_carlo_report.txt",
            "simulation_results"} <= set(os.listdir(out_dir))
    assert os.path.getsize(os.path.join(out_dir, "monte_carlo_distributions.png")) > 10000
    report = json.load(open(os.path.join(out_dir, "monte_carlo_report.json")))
    assert report["simulation_summary"]["total_simulations"] == res["n_samples"]
    dirs = {out_dir}
    for method, name in ((mc.plot_trajectory_cloud_3d, "monte_carlo_trajectories_3d.png"),
                         (mc.plot_trajectory_cloud, "monte_carlo_trajectories.png")):
        d = method(res)
        assert os.path.getsize(os.path.join(d, name)) > 10000
        dirs.add(d)
    d = mc.plot_landing_dispersion(res)
    assert {"landing_dispersion.json", "monte_carlo_landing.png"} <= set(os.listdir(d))
    saved = json.load(open(os.path.join(d, "landing_dispersion.json")))
    assert saved["n_samples"] == res["n_samples"] and saved["count"] <= res["n_samples"]
    dirs.add(d)
    root = os.path.realpath(str(tmp_path))
    assert all(os.path.realpath(x).startswith(root) for x in dirs)


# ------------------------------------------------------------------ stream order
def test_distributions_are_ordered_behind_the_stream(engine):
    """The summary is produced on a side stream; the current stream waits for it on the device and the three calls are
    enqueued there with no host synchronisation in between.  A dependency check, run once."""
    rng = np.random.RandomState(3)
    n = 1 << 18
    base = np.zeros((16, n))
    base[_abi.SUM_APOGEE_ALT] = rng.normal(25000, 20000, n)
    base[_abi.SUM_RANGE] = np.abs(rng.normal(50000, 90000, n))
    base[_abi.SUM_IMPACT_X] = rng.normal(100, 2000, n)
    base[_abi.SUM_IMPACT_Y] = rng.normal(-300, 900, n)
    src = torch.from_numpy(base).to(engine.device)
    ds = torch.full((16, n), float("nan"), dtype=torch.float64, device=engine.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=engine.device)
    with torch.cuda.stream(side):
        tmp = src
        for _ in range(40):          # some work in front of the copy, all on the side stream
            tmp = tmp * 1.0
        ds.copy_(tmp)
    torch.cuda.current_stream(engine.device).wait_stream(side)
    edges, counts, info = engine.histogram(ds, rows=[_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE], bins=50)
    assert info["counted"] == [n, n]
    check_hist(engine, ds, None, base, None, [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE], 50)
    check_hist2d(engine, ds, None, base, None, _abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, 50)
    check_dispersion(engine, ds, None, base, None, _abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y, (0.0, 0.0))


# ------------------------------------------------------------------ the Python layer
def test_python_layer_refuses_what_the_kernels_cannot_take(engine):
    ok = torch.zeros((16, 8), dtype=torch.float64, device=engine.device)
    for method in (engine.histogram, engine.histogram2d, engine.dispersion):
        for bad in (ok.cpu(), ok.float(), ok[:, ::2], ok[:15], ok.t().contiguous()):
            with pytest.raises(ValueError):
                method(bad)
        for bad_mask in (torch.zeros(8, dtype=torch.int32, device=engine.device),
                         torch.zeros(9, dtype=torch.uint8, device=engine.device), torch.zeros(8, dtype=torch.uint8)):
            with pytest.raises(ValueError):
                method(ok, bad_mask)
    with pytest.raises(_abi.ErplError, match="twice"):
        engine.histogram(ok, rows=[1, 1])
    with pytest.raises(_abi.ErplError, match=r"bins\[0\] = 1025"):
        engine.histogram(ok, rows=[1], bins=1025)
    with pytest.raises(_abi.ErplError, match="bins_y = 257"):
        engine.histogram2d(ok, bins=(4, 257))
    with pytest.raises(_abi.ErplError, match=r"level\[0\]"):
        engine.dispersion(ok, levels=[1.0])
    edges, counts, info = engine.histogram(ok, rows=[5], bins=4)          # a constant row: (-0.5, 0.5), bin 2
    assert list(edges[0]) == [-0.5, -0.25, 0.0, 0.25, 0.5] and list(counts[0]) == [0, 0, 8, 0]


# ------------------------------------------------------------------ the workspaces on one engine: regrow and shared use
def test_workspaces_regrow_and_are_shared_like_on_fresh_engines():
    """analyze, dispersion and histogram in turn on ONE engine, at 257 and 4099 samples (2 and 17 workgroups of
    ERPL_ANA_BLOCK, one sample past a block boundary): the reason bytes and the miss-distance row grow between the calls,
    and dispersion without a mask takes the reason bytes `analyze` has just filled as its row of zeros.  The library
    promises repeatable bytes, so every result equals what the same single call gives on a fresh engine - no tolerance."""
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    dev = torch.device("cuda", 0)
    data = {}
    for n in (257, 4099):
        summ, status = H.synthetic_summary(n, 40 + n)
        data[n] = (torch.from_numpy(summ).to(dev), torch.from_numpy(status).to(dev))

    def analyze(eng, n, reasons):
        res, why = eng.analyze(*data[n], reasons=reasons)
        assert 0 < res.n_valid < n
        return bytes(res), None if why is None else why.cpu().numpy()

    def dispersion(eng, n, _):
        return eng.dispersion(data[n][0], None, miss=False)

    def histogram(eng, n, _):
        return eng.histogram(data[n][0])

    calls = [(analyze, 257, True), (analyze, 4099, True), (dispersion, 257, None), (dispersion, 4099, None),
             (histogram, 4099, None), (analyze, 257, False)]
    one = TrajectoryEngine(dev)
    got = [fn(one, n, arg) for fn, n, arg in calls]
    one.close()
    for (fn, n, arg), g in zip(calls, got):
        fresh = TrajectoryEngine(dev)
        ref = fn(fresh, n, arg)
        fresh.close()
        if fn is analyze:
            assert g[0] == ref[0] and (g[1] is None) == (ref[1] is None) and (g[1] is None or np.array_equal(g[1], ref[1])), n
        elif fn is dispersion:
            assert g["count"] > 0 and H.same_nested(g, ref), (n, g, ref)
        else:
            for j in range(len(DEFAULT_ROWS)):
                assert np.array_equal(g[0][j], ref[0][j]) and np.array_equal(g[1][j], ref[1][j]), (n, j)
            assert H.same_nested(g[2], ref[2]), (n, g[2], ref[2])
