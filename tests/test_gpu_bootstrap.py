"""erpl_mc_bootstrap on the device against NumPy with the tests' own Philox (philox_ref) on host copies of the same tensors.

Per replicate and statistic, from `replicates_out`:
  quantiles   bit for bit the formula of erpl_mc_analyze on the two order statistics NumPy finds in x[idx] (q = 0, q = 1 and
              the median of an odd m are an order statistic itself, bit for bit too - but for an order statistic -0.0, which
              the formula returns as -0.0 + 0.0 = +0.0, here as in erpl_mc_analyze).  The order statistics are those of
              np.sort with -0.0 below +0.0: np.sort leaves the order of the two zeros open, the device's keys do not.
  mean        within m * 2^-53 * mean|x[idx]| of np.mean: any summation order of m terms.
  std         within 4 m * 2^-53 relative of the two-pass np.std.
Per statistic: count / n_masked / n_non_finite exact, finite == B, rep_mean / se / lo / hi against NumPy on the returned
replicates at 1e-12 relative (the bar of test_gpu_analysis.py), estimate bit for bit erpl_mc_analyze's on inputs whose
non-finite samples are all masked.

The all-equal row holds 7.25: k * 7.25 is exact for every k in reach, so sum / count is 7.25 in every summation order and
`lo == hi == estimate` can be asked to the bit (for a value such as 0.1 the mean of the population and the mean of a
replicate are each sum / count in their own order and may differ in the last bit)."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import helpers as H
import philox_ref

pytestmark = pytest.mark.gpu

TOL = 1e-12
U = 2.0 ** -53
ROWS = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.BOOT_ROW_EXTRA, _abi.SUM_FLIGHT_TIME]   # row 4 (range) is the tied one
Q8 = [0.0, 1.0, 0.5, 0.05, 0.25, 0.75, 0.95, 0.999]
TIED = np.array([-2.5, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0, 7.25])
# (population m, replicates B, quantiles): one, two and three digit sweeps, odd m (the last Philox call half used), m below
# one workgroup and below one wave, B = 300 where m <= 4 099, n_q in {0, 1, 8}
CASES = [(1, 3, Q8), (2, 64, [0.5]), (63, 1, Q8), (64, 3, []), (65, 64, Q8), (255, 300, Q8), (256, 3, [0.5]), (257, 64, Q8),
         (4099, 300, Q8), (4099, 64, []), (65535, 3, Q8), (65536, 64, [1.0]), (65537, 1, Q8), (70001, 64, Q8),
         (70001, 3, [0.0])]


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


def dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def bits(a):
    """The 64 bits of every double of `a`: an int for a scalar, a uint64 array otherwise."""
    a = np.asarray(a, dtype=np.float64)
    out = np.ascontiguousarray(a).reshape(-1).view(np.uint64)
    return int(out[0]) if a.ndim == 0 else out.reshape(a.shape)


def total_sort(x):
    """np.sort of finite doubles with -0.0 below +0.0 (the order of key_of_signed)."""
    b = bits(x)
    key = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    key = np.sort(key)
    return np.where(key >> np.uint64(63) != 0, key & np.uint64((1 << 63) - 1), ~key).view(np.float64)


def make_inputs(m, seed):
    """A [16, n] summary, an extra row and a mask whose population - mask byte 0, rows ROWS all finite - has exactly m
    members: m + 7 samples, 3 of them masked (one of those non-finite too) and 4 unmasked with a NaN or an infinity."""
    rng = np.random.default_rng(seed)
    n = m + 7
    summ = rng.normal(size=(_abi.SUMMARY_DIM, n))
    summ[_abi.SUM_APOGEE_ALT] = rng.lognormal(9.0, 0.3, n)
    summ[_abi.SUM_FLIGHT_TIME] = rng.lognormal(4.0, 0.3, n)
    summ[_abi.SUM_RANGE] = TIED[rng.integers(0, len(TIED), n)]
    extra = rng.lognormal(6.0, 0.8, n)
    where = rng.permutation(n)[:7]
    mask = np.zeros(n, dtype=np.uint8)
    mask[where[:3]] = [1, 4, 32]
    summ[_abi.SUM_FLIGHT_TIME, where[2]] = np.nan
    summ[_abi.SUM_APOGEE_ALT, where[3]] = np.nan
    summ[_abi.SUM_APOGEE_ALT, where[4]] = np.inf
    extra[where[5]] = -np.inf
    summ[_abi.SUM_RANGE, where[6]] = np.nan
    return summ, extra, mask


def population(summ, extra, mask, rows):
    X = np.vstack([extra if r == _abi.BOOT_ROW_EXTRA else summ[r] for r in rows])
    masked = np.zeros(X.shape[1], dtype=bool) if mask is None else mask != 0
    fin = np.isfinite(X).all(axis=0)
    pop = ~masked & fin
    return X[:, pop], int(masked.sum()), int((~masked & ~fin).sum())


def interpolate(s, q):
    """The quantile formula of erpl_mc_analyze on an ascending array."""
    m = len(s)
    pos = q * float(m - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, m - 1)
    return s[lo] + (s[hi] - s[lo]) * (pos - lo)


def close(got, want, tol=TOL):
    if np.isnan(want):
        assert np.isnan(got)
        return
    assert abs(got - want) <= tol * abs(want), (got, want)


def check_replicates(P, rep, seed, quantiles, which=None):
    """Every replicate in rep [n_stats, B] (or those in `which`) against NumPy on the drawn values."""
    R, m = P.shape
    ns, B = 2 + len(quantiles), rep.shape[1]
    worst_mean = worst_std = 0.0
    for b in (range(B) if which is None else which):
        idx = philox_ref.indices(seed, b, m)
        assert idx.min() >= 0 and idx.max() < m
        for j in range(R):
            x = P[j, idx]
            got = rep[j * ns:(j + 1) * ns, b]
            bound = m * U * np.mean(np.abs(x))
            assert abs(got[0] - np.mean(x)) <= bound, (j, b, got[0], np.mean(x))
            worst_mean = max(worst_mean, abs(got[0] - np.mean(x)) / bound if bound else 0.0)
            std = np.std(x)
            assert abs(got[1] - std) <= 4 * m * U * std, (j, b, got[1], std)
            worst_std = max(worst_std, abs(got[1] - std) / (4 * m * U * std) if std else 0.0)
            s = total_sort(x)
            want = np.array([interpolate(s, q) for q in quantiles], dtype=np.float64)
            assert np.array_equal(bits(got[2:]), bits(want)), (j, b, got[2:], want)
            for i, q in enumerate(quantiles):
                pos = q * float(m - 1)
                if pos == np.floor(pos):   # an order statistic itself (a -0.0 leaves the formula as -0.0 + 0.0 = +0.0)
                    assert got[2 + i] == s[int(pos)] and (s[int(pos)] == 0.0 or bits(got[2 + i]) == bits(s[int(pos)]))
    return worst_mean, worst_std


def check_summary(out, rep, level):
    """rep_mean / se / lo / hi / finite of every statistic against NumPy on the returned replicates."""
    B = rep.shape[1]
    flat = [s for row in out["stats"] for s in [row["mean"], row["std"]] + row["quantiles"]]
    assert len(flat) == rep.shape[0]
    tail = (1.0 - level) / 2
    for s, theta in zip(flat, rep):
        assert s["finite"] == B
        if theta.min() == theta.max():
            assert s["se"] == 0.0 and s["rep_mean"] == theta[0]
        else:
            close(s["rep_mean"], np.mean(theta))
            close(s["se"], np.std(theta, ddof=1))
        srt = np.sort(theta)
        close(s["lo"], interpolate(srt, tail))
        close(s["hi"], interpolate(srt, 1.0 - tail))


@pytest.mark.parametrize("m,B,quantiles", CASES, ids=[f"m{m}-B{B}-q{len(q)}" for m, B, q in CASES])
def test_replicates_and_their_summary_against_numpy(engine, m, B, quantiles):
    summ, extra, mask = make_inputs(m, 1000 + m)
    seed = 77 + m
    out = engine.bootstrap(dev(engine, summ), dev(engine, mask), rows=ROWS, quantiles=quantiles, replicates=B, level=0.9,
                           seed=seed, extra=dev(engine, extra), want_replicates=True)
    P, n_masked, n_non_finite = population(summ, extra, mask, ROWS)
    assert P.shape[1] == m
    assert (out["n"], out["count"], out["n_masked"], out["n_non_finite"]) == (m + 7, m, n_masked, n_non_finite)
    assert (n_masked, n_non_finite) == (3, 4) and out["rows"] == ROWS and out["replicates"] == B
    rep = out["replicate_values"].cpu().numpy()
    assert rep.shape == (4 * (2 + len(quantiles)), B)
    worst = check_replicates(P, rep, seed, quantiles)
    print(f"m {m} B {B}: mean error {worst[0]:.3g} of its bound, std error {worst[1]:.3g} of its bound")
    check_summary(out, rep, 0.9)
    # the estimates: the statistics of the population itself
    for j, row in enumerate(out["stats"]):
        close(row["mean"]["estimate"], np.mean(P[j]))
        close(row["std"]["estimate"], np.std(P[j]))
        s = total_sort(P[j])
        for i, q in enumerate(quantiles):
            assert bits(row["quantiles"][i]["estimate"]) == bits(interpolate(s, q))
    if m == 1:   # every replicate is that value
        for j in range(4):
            ns = 2 + len(quantiles)
            assert np.all(bits(rep[j * ns]) == bits(P[j, 0])) and np.all(rep[j * ns + 1] == 0.0)
            assert np.all(bits(rep[j * ns + 2:(j + 1) * ns]) == bits(P[j, 0]))
            for s in [out["stats"][j]["mean"]] + out["stats"][j]["quantiles"]:
                assert s["se"] == 0.0 and bits(s["lo"]) == bits(s["hi"]) == bits(s["estimate"]) == bits(P[j, 0])


def test_estimates_are_the_bits_of_erpl_mc_analyze(engine):
    """Non-finite values in the filter rows only: erpl_mc_analyze masks them all, so its population of every row is the
    bootstrap's."""
    n = 70003
    rng = np.random.default_rng(5)
    summ = rng.normal(size=(_abi.SUMMARY_DIM, n))
    summ[_abi.SUM_APOGEE_ALT] = rng.lognormal(9.0, 0.3, n)      # a few below 100 m or above 80 km: filtered
    summ[_abi.SUM_RANGE] = TIED[rng.integers(0, len(TIED), n)] * 1000.0
    summ[_abi.SUM_FLIGHT_TIME] = rng.lognormal(4.0, 0.3, n)
    summ[_abi.SUM_APOGEE_ALT, [3, 70000]] = [np.nan, 90000.0]
    summ[_abi.SUM_RANGE, 11] = np.inf
    summ[_abi.SUM_FLIGHT_TIME, [64, 65]] = [-np.inf, 601.0]
    rows, quantiles = [_abi.SUM_FLIGHT_TIME, _abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_MAX_SPEED], Q8
    d = dev(engine, summ)
    res, why = engine.analyze(d, None, rows=rows, quantiles=quantiles, reasons=True)
    assert 0 < res.n_valid < n
    out = engine.bootstrap(d, why, rows=rows, quantiles=quantiles, replicates=3, seed=1)
    assert out["count"] == res.n_valid and out["n_non_finite"] == 0 and out["n_masked"] == res.n_outliers
    for j in range(4):
        r, s = res.row[j], out["stats"][j]
        assert r.count == res.n_valid
        assert bits(s["mean"]["estimate"]) == bits(r.mean) and bits(s["std"]["estimate"]) == bits(r.std)
        assert np.array_equal(bits([p["estimate"] for p in s["quantiles"]]), bits(list(r.quantile[:8])))


def test_repeatable_and_independent_of_the_number_of_replicates_and_of_the_stream(engine):
    summ, extra, mask = make_inputs(4099, 9)
    args = (dev(engine, summ), dev(engine, mask))
    kw = dict(rows=ROWS, quantiles=Q8, extra=dev(engine, extra), want_replicates=True)

    def frozen(out):
        return repr([(k, v) for k, v in out.items() if k != "replicate_values"]), out["replicate_values"].cpu().numpy()

    a, rep_a = frozen(engine.bootstrap(*args, replicates=300, seed=31, **kw))
    b, rep_b = frozen(engine.bootstrap(*args, replicates=300, seed=31, **kw))
    assert a == b and np.array_equal(bits(rep_a), bits(rep_b))
    _, rep_c = frozen(engine.bootstrap(*args, replicates=300, seed=32, **kw))
    assert not np.array_equal(rep_a[0], rep_c[0]) and not np.array_equal(rep_a[2], rep_c[2])
    _, rep_10 = frozen(engine.bootstrap(*args, replicates=10, seed=31, **kw))
    assert np.array_equal(bits(rep_10), bits(rep_a[:, :10]))
    side = torch.cuda.Stream(engine.device)
    side.wait_stream(torch.cuda.current_stream(engine.device))
    with torch.cuda.stream(side):
        d, rep_d = frozen(engine.bootstrap(*args, replicates=300, seed=31, **kw))
    side.synchronize()
    assert d == a and np.array_equal(bits(rep_d), bits(rep_a))


def test_nothing_counted_is_nan_and_no_error(engine):
    summ, extra, _ = make_inputs(257, 3)
    mask = np.full(summ.shape[1], 2, dtype=np.uint8)
    out = engine.bootstrap(dev(engine, summ), dev(engine, mask), rows=ROWS, quantiles=[0.5], replicates=5,
                           extra=dev(engine, extra), want_replicates=True)
    assert (out["count"], out["n_masked"], out["n_non_finite"]) == (0, summ.shape[1], 0)
    assert np.isnan(out["replicate_values"].cpu().numpy()).all()
    for row in out["stats"]:
        for s in [row["mean"], row["std"]] + row["quantiles"]:
            assert s["finite"] == 0 and all(np.isnan(s[k]) for k in ("estimate", "rep_mean", "se", "lo", "hi"))
    # no mask, but a row without a finite value
    summ[_abi.SUM_RANGE] = np.nan
    out = engine.bootstrap(dev(engine, summ), None, rows=[_abi.SUM_RANGE], quantiles=[], replicates=1)
    assert (out["count"], out["n_masked"], out["n_non_finite"]) == (0, 0, summ.shape[1])
    assert np.isnan(out["stats"][0]["mean"]["se"]) and out["stats"][0]["std"]["finite"] == 0


def test_all_equal_row_has_no_spread(engine):
    summ, _, mask = make_inputs(4099, 4)
    summ[_abi.SUM_RANGE] = 7.25
    out = engine.bootstrap(dev(engine, summ), dev(engine, mask), rows=[_abi.SUM_RANGE, _abi.SUM_APOGEE_ALT], quantiles=Q8,
                           replicates=64, seed=6)
    flat = out["stats"][0]
    assert flat["std"]["estimate"] == 0.0 and flat["std"]["se"] == 0.0 and flat["std"]["lo"] == flat["std"]["hi"] == 0.0
    for s in [flat["mean"]] + flat["quantiles"]:
        assert s["se"] == 0.0 and s["lo"] == s["hi"] == s["estimate"] == s["rep_mean"] == 7.25 and s["finite"] == 64
    assert out["stats"][1]["mean"]["se"] > 0.0   # the row beside it is alive


def test_standard_error_of_the_mean_is_sigma_over_root_m(engine):
    """The bootstrap variance of the mean is exactly var(x) / m; an se estimated from B replicates has a relative sd of
    1 / sqrt(2 B): five of those, 1 +- 0.079 at B = 2 000.  (The NumPy recipe gives 1.012 for this seed.)"""
    m, B = 4099, 2000
    rng = np.random.default_rng(2024)
    summ = rng.normal(size=(_abi.SUMMARY_DIM, m))
    summ[_abi.SUM_APOGEE_ALT] = rng.lognormal(9.0, 0.3, m)
    out = engine.bootstrap(dev(engine, summ), None, rows=[_abi.SUM_APOGEE_ALT], quantiles=[0.5], replicates=B, seed=2024)
    x = summ[_abi.SUM_APOGEE_ALT]
    s = out["stats"][0]["mean"]
    ratio = s["se"] / (np.std(x) / np.sqrt(m))
    print(f"se of the mean / (sigma / sqrt(m)) = {ratio:.4f}")
    assert abs(ratio - 1.0) <= 5.0 / np.sqrt(2 * B)
    assert s["lo"] < s["estimate"] < s["hi"] and s["finite"] == B
    close(s["estimate"], np.mean(x))


# ------------------------------------------------------------------ the Python layer on real flights
@pytest.fixture(scope="module")
def analyzer():
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    return MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)


@pytest.fixture(scope="module")
def flights(analyzer):
    return analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 512, precision="f64_fast")


def test_confidence_intervals_of_a_real_batch(engine, analyzer, flights):
    summ = flights["summary"]
    ci = analysis.confidence_intervals(summ, status=flights["status"], engine=engine, replicates=200, seed=3)
    st = analysis.native_statistics(summ, status=flights["status"], engine=engine)
    assert ci["n_samples"] == st["n_samples"] == ci["count"] and ci["replicates"] == 200 and ci["level"] == 0.95
    for name in ("apogee_altitude", "range", "flight_time"):
        row = ci[name]
        assert bits(row["mean"]["estimate"]) == bits(st[name]["mean"]) and bits(row["std"]["estimate"]) == bits(st[name]["std"])
        assert np.array_equal(bits([p["estimate"] for p in row["percentiles"]]), bits(st[name]["percentiles"]))
        for s in [row["mean"], row["std"]] + row["percentiles"]:
            assert set(s) == {"estimate", "se", "lo", "hi"} and s["lo"] <= s["estimate"] <= s["hi"] and s["se"] >= 0.0
        # sigma / sqrt(m), at five relative standard deviations of an se from 200 replicates
        assert abs(row["mean"]["se"] / (st[name]["std"] / np.sqrt(ci["count"])) - 1.0) <= 5.0 / np.sqrt(2 * 200)
    # the samples replicate 0 drew, by name
    idx = analysis.bootstrap_indices(3, 0, ci["count"])
    assert np.array_equal(idx, philox_ref.indices(3, 0, ci["count"]))
    # the analyzer's method takes the dict of the device run
    again = analyzer.confidence_intervals(flights, replicates=200, seed=3)
    assert H.same_nested(again, ci)


def test_cep_interval_carries_the_cep_of_landing_dispersion(engine, flights):
    summ = flights["summary"]
    disp = analysis.landing_dispersion(summ, status=flights["status"], engine=engine)
    cep = analysis.cep_interval(summ, status=flights["status"], engine=engine, replicates=200, seed=8)
    assert cep["count"] == disp["miss"]["count"] and cep["q"] == [0.5, 0.9, 0.95, 0.99]
    assert bits(cep["cep"]["estimate"]) == bits(disp["cep"])
    assert np.array_equal(bits([p["estimate"] for p in cep["quantiles"]]), bits(disp["miss"]["quantiles"]))
    assert bits(cep["mean"]["estimate"]) == bits(disp["miss"]["mean"])
    assert cep["cep"]["lo"] <= cep["cep"]["estimate"] <= cep["cep"]["hi"] and cep["cep"]["se"] > 0.0
