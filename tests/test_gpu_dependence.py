"""erpl_mc_dependence on the device against the NumPy / SciPy yardstick of dependence_ref on host copies of the same tensors.

Equal: the counts, the tables, the class counts, delta_num, classes_used, cells_used and exceed (of mi: equal wherever its
tolerance decides the comparison, see compare).  Equal to the bit: delta,
ks_max, ks_median, their null values, null_mean and null_hi - formed from the same integers by the same IEEE operations.
mi and its null values: within 4 K log(M H) 2^-52 absolute, K the non-empty cells of the table (the rounding bound of K terms
of at most log(M H), with room for a 2-ulp device log).  The class means: within u sum|y| + 2 u |mean| of the long double mean
(u = 2^-53: any summation order of n_c terms is within n_c u sum|y| of the exact sum; divided by n_c, one rounding of the
quotient and one of the reference to a double).  The class std: the
centre is off by at most that e, which moves a root-mean-square by at most e, and n_c + 4 roundings of
positive terms under a square root: e + (n_c + 4) 2^-52 std.  eta2, eta2_adj, f_stat, row_mean, row_ss: 1e-12 relative to
the long double evaluation (plus 1e-12 absolute on eta2 and eta2_adj, which live on [0, 1]), on inputs whose row_ss is at
least a thousandth of sum y^2 (asserted).  x_lo, x_hi, x_median: exact."""
import math

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import dependence_ref as ref
import helpers as H
import philox_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EXTRA = _abi.DEP_ROW_EXTRA
EXACT = ("delta", "ks_max", "ks_median")


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
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make_inputs(n, F, rows, seed, dirty=True):
    """factors [F, n], a [16, n] summary, an extra row and a mask.  The rows depend on the factors in a non-monotone way
    (so that the measures are of order one for some pairs and null for others) on top of an offset.  dirty: three
    samples masked, a NaN and an infinity in a factor, an infinity and a NaN in a row (n >= 16)."""
    rng = np.random.default_rng(seed)
    fac = rng.normal(size=(F, n))
    summ = rng.normal(size=(_abi.SUMMARY_DIM, n))
    extra = rng.normal(size=n)
    for k, r in enumerate(rows):
        y = 5.0 + np.sin(2.0 * fac[k % F]) + 0.5 * fac[(k + 1) % F] ** 2 + 0.3 * rng.normal(size=n)
        if r == EXTRA:
            extra[:] = y
        else:
            summ[r] = y
    mask = np.zeros(n, dtype=np.uint8)
    if dirty and n >= 16:
        where = rng.permutation(n)[:7]
        mask[where[:3]] = [1, 4, 32]
        fac[0, where[3]], fac[F - 1, where[4]] = np.nan, np.inf
        target = extra if rows[-1] == EXTRA else summ[rows[-1]]
        target[where[5]] = -np.inf
        summ[rows[0], where[6]] = np.nan
        summ[rows[0], where[0]] = np.nan                 # masked as well: counted as masked
    return fac, summ, extra, mask


def rows_of(summ, extra, rows):
    return np.vstack([extra if r == EXTRA else summ[r] for r in rows])


def run(engine, fac, summ, extra, mask, rows, **kw):
    kw.setdefault("want_tables", True)
    kw.setdefault("want_null", kw.get("shifts", 200) > 0)
    return engine.dependence(dev(engine, fac), dev(engine, summ), dev(engine, mask) if mask is not None else None, rows=rows,
                             extra=dev(engine, extra) if EXTRA in rows else None, **kw)


def compare(out, want, fac, ys, mask, M, H, P, what):
    masked = np.zeros(fac.shape[1], dtype=bool) if mask is None else mask != 0
    fin = np.isfinite(fac).all(axis=0) & np.isfinite(ys).all(axis=0)
    assert (out["count"], out["n_masked"], out["n_non_finite"]) == (int((~masked & fin).sum()), int(masked.sum()),
                                                                    int((~masked & ~fin).sum())), what
    m = want["count"]
    assert out["count"] == m, what
    for key in ("tables", "delta_num", "classes_used", "cells_used"):
        assert np.array_equal(out[key], want[key]), (what, key)
    assert np.array_equal(out["class_stats"][..., 0], want["class_stats"][..., 0]), what
    nulls = P > 0 and m >= 2
    bound = 4.0 * want["mi_cells"] * math.log(M * H) * 2.0 ** -52           # [R, F, 1 + P]
    for key in ref.MEASURES:
        if key in EXACT:
            assert np.array_equal(out[key]["exceed"], want[key]["exceed"]), (what, key)
            for field in ("estimate", "null_mean", "null_hi"):
                assert same_bits(out[key][field], want[key][field]), (what, key, field, out[key][field], want[key][field])
    if m > 0:
        err = np.abs(out["mi"]["estimate"] - want["mi"]["estimate"])
        print(f"{what}: mi estimate worst share of its bound {np.max(err / np.maximum(bound[..., 0], 1e-300)):.3f}")
        assert np.all(err <= bound[..., 0]), (what, err, bound[..., 0])
    else:
        assert np.isnan(out["mi"]["estimate"]).all() and np.isnan(out["delta"]["estimate"]).all(), what
    if "null_values" in out:
        got, exp = out["null_values"], want["null_values"]
        if nulls:
            assert same_bits(got[:, :, :3], exp[:, :, :3]), what
            assert np.all(np.abs(got[:, :, 3] - exp[:, :, 3]) <= bound[..., 1:]), what
            # exceed of mi: equal wherever the bounds decide it - a null value closer to the estimate than the two bounds
            # together may count or not (64 x 64 cells over a thousand members: many tables have the same mi in exact terms)
            gap = exp[:, :, 3] - want["mi"]["estimate"][..., None]
            both = bound[..., 1:] + bound[..., :1]
            assert np.all((gap > both).sum(axis=-1) <= out["mi"]["exceed"]), what
            assert np.all(out["mi"]["exceed"] <= (gap >= -both).sum(axis=-1)), what
            # ... and the count of the returned null values that reach the returned estimate, exactly
            assert np.array_equal(out["mi"]["exceed"], (got[:, :, 3] >= out["mi"]["estimate"][..., None]).sum(axis=-1)), what
            worst = bound[..., 1:].max(axis=-1)
            for field in ("null_mean", "null_hi"):
                assert np.all(np.abs(out["mi"][field] - want["mi"][field]) <= worst), (what, field)
        else:
            assert np.isnan(got).all(), what
    if not nulls:
        for key in ref.MEASURES:
            assert np.isnan(out[key]["null_mean"]).all() and np.isnan(out[key]["null_hi"]).all(), (what, key)
            assert not out[key]["exceed"].any(), (what, key)
    # the variance share
    cs, cw = out["class_stats"], want["class_stats"]
    assert np.array_equal(np.isnan(cs), np.isnan(cw)), what
    assert np.array_equal(cs[..., 3:], cw[..., 3:], equal_nan=True), (what, "x_lo / x_hi / x_median")
    if m == 0:
        for key in ("eta2", "eta2_adj", "f_stat", "row_mean", "row_ss"):
            assert np.isnan(out[key]).all(), (what, key)
        return
    R, F = out["eta2"].shape
    for j in range(R):
        y = ys[j][~masked & fin]
        flat = y.min() == y.max()
        assert abs(out["row_mean"][j] - want["row_mean"][j]) <= 1e-12 * abs(want["row_mean"][j]), what
        if not flat:
            assert want["row_ss"][j] >= 1e-3 * float((y * y).sum()) or m < 3, (what, "row_ss is tiny against sum y^2")
            assert abs(out["row_ss"][j] - want["row_ss"][j]) <= 1e-12 * want["row_ss"][j], what
        for f in range(F):
            vs = want["share"][j][f]
            used = vs["count"] > 0
            n_c = vs["count"][used].astype(np.float64)
            mean_ref = vs["mean"][used].astype(np.float64)
            e = U * vs["sum_abs"][used].astype(np.float64) + 2 * U * np.abs(mean_ref)
            assert np.all(np.abs(cs[j, f, used, 1] - mean_ref) <= e), (what, j, f, "class means")
            std_ref = cw[j, f, used, 2]
            assert np.all(np.abs(cs[j, f, used, 2] - std_ref) <= e + (n_c + 4) * 2.0 ** -52 * std_ref), (what, j, f, "class std")
            for key, floor in (("eta2", 1e-12), ("eta2_adj", 1e-12), ("f_stat", 0.0)):
                g, w = out[key][j, f], want[key][j, f]
                if np.isnan(w):
                    assert np.isnan(g), (what, key, j, f, g)
                elif flat or want["classes_used"][j, f] < 2:
                    assert g == w, (what, key, j, f, g, w)
                else:
                    assert abs(g - w) <= 1e-12 * abs(w) + floor, (what, key, j, f, g, w)


def check(engine, fac, summ, extra, mask, rows, M, H, P, seed=0, level=0.95, what=""):
    out = run(engine, fac, summ, extra, mask, rows, classes=M, cells=H, shifts=P, seed=seed, level=level)
    ys = rows_of(summ, extra, rows)
    want = ref.dependence(fac, ys, mask, classes=M, cells=H, shifts=P, level=level, seed=seed)
    compare(out, want, fac, ys, mask, M, H, P, what)
    return out, want


# n: below and around one wave and one workgroup, above one; every (M, H) corner; P in {0, 1, 7}; R = 2 with row 16
@pytest.mark.parametrize("n, M, H, P", [(1, 2, 2, 7), (2, 3, 64, 1), (255, 64, 3, 7), (256, 64, 64, 0), (257, 2, 2, 1),
                                        (1025, 3, 64, 7)])
def test_small_shapes_against_the_yardstick(engine, n, M, H, P):
    rows = [_abi.SUM_RANGE, EXTRA]
    fac, summ, extra, mask = make_inputs(n, 2, rows, seed=n)
    out, want = check(engine, fac, summ, extra, mask if n >= 16 else None, rows, M, H, P, seed=n, what=f"n {n}")
    assert out["count"] == (n - 7 if n >= 16 else n)


def test_many_factors_and_rows(engine):
    """F = 32 and R = 4, row 16 among them, 64 x 64 classes: 128 pairs, every one its own workgroup column."""
    rows = [_abi.SUM_APOGEE_ALT, EXTRA, _abi.SUM_MAX_SPEED, _abi.SUM_RANGE]
    fac, summ, extra, mask = make_inputs(1025, 32, rows, seed=5)
    check(engine, fac, summ, extra, mask, rows, 64, 64, 7, seed=3, level=0.5, what="F 32 R 4")


@pytest.mark.parametrize("m", [4097, 262144 + 257])
def test_more_than_one_tile_and_more_than_one_grid(engine, m):
    """m = one more than a tile of the table pass (256 threads x 16 members), and m beyond the 1024 x 256 members the grid of
    the streaming passes covers in one step (one more than a multiple of 256 as well)."""
    rows = [_abi.SUM_FLIGHT_TIME]
    fac, summ, extra, mask = make_inputs(m + 7, 1, rows, seed=m)
    out, _ = check(engine, fac, summ, extra, mask, rows, 16, 16, 1, seed=9, what=f"m {m}")
    assert out["count"] == m


def shifts_with_both_ends(m, P):
    """A seed whose P shifts of a population of m include 1 and m - 1 (searched on the CPU with the tests' own Philox)."""
    for seed in range(100000):
        s = ref.shifts_of(seed, m, P)
        if 1 in s and m - 1 in s:
            return seed
    raise AssertionError("no such seed")


def test_the_shifts_at_both_ends(engine):
    m, P = 21, 7
    seed = shifts_with_both_ends(m, P)
    rows = [_abi.SUM_RANGE]
    fac, summ, extra, _ = make_inputs(m, 1, rows, seed=2, dirty=False)
    out, want = check(engine, fac, summ, extra, None, rows, 3, 5, P, seed=seed, what=f"seed {seed}")
    assert 1 in want["shift_values"] and m - 1 in want["shift_values"]
    assert [int(philox_ref.indices(seed, 0, m - 1, p, 1)[0]) + 1 for p in range(P)] == want["shift_values"]


def test_ties_constant_factor_and_constant_row(engine):
    """Factor 0: integers 0..4 (tied values share a class, classes stay empty); factor 1: constant, -0.0 and +0.0 mixed
    (class M div 2 alone, every measure exactly 0, eta2 = 0); row 1: constant (eta2 NaN, one cell)."""
    n, M, Hc = 1001, 7, 4
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE]
    fac, summ, extra, mask = make_inputs(n, 3, rows, seed=8)
    fin = np.isfinite(fac[0])
    fac[0, fin] = (np.arange(n) % 5)[fin]
    fac[1] = np.where(np.arange(n) % 3 == 0, -0.0, 0.0)
    summ[_abi.SUM_APOGEE_ALT] = 10.0 + fac[2] ** 2 + np.where(fin, fac[0], 0.0)
    summ[_abi.SUM_RANGE] = 7.5
    out, want = check(engine, fac, summ, extra, mask, rows, M, Hc, 7, seed=4, what="ties")
    assert list(out["classes_used"][0]) == [5, 1, M] and list(out["cells_used"][:, 0]) == [Hc, 1]
    assert np.all(out["tables"][0, 1, [c for c in range(M) if c != M // 2]] == 0)
    for key in ref.MEASURES:
        assert out[key]["estimate"][0, 1] == 0.0 and out[key]["exceed"][0, 1] == 7
        assert np.all(out[key]["estimate"][1] == 0.0)
    assert out["delta_num"][0, 1] == 0 and out["eta2"][0, 1] == 0.0 and np.isnan(out["eta2_adj"][0, 1])
    assert np.isnan(out["eta2"][1]).all() and np.isnan(out["f_stat"][1]).all()


def test_empty_and_single_member_populations(engine):
    rows = [_abi.SUM_RANGE, EXTRA]
    fac, summ, extra, _ = make_inputs(40, 2, rows, seed=1, dirty=False)
    mask = np.ones(40, dtype=np.uint8)
    out, _ = check(engine, fac, summ, extra, mask, rows, 4, 4, 7, what="m 0")
    assert out["count"] == 0 and not out["tables"].any() and not out["delta_num"].any()
    assert not out["class_stats"][..., 0].any() and np.isnan(out["class_stats"][..., 1:]).all()
    mask[17] = 0
    out, _ = check(engine, fac, summ, extra, mask, rows, 4, 4, 7, what="m 1")
    assert out["count"] == 1 and out["tables"].sum() == 4 and np.all(out["tables"][:, :, 2, 2] == 1)
    assert np.all(out["delta"]["estimate"] == 0.0) and np.isnan(out["delta"]["null_mean"]).all()


def flat(out):
    """Every number of a result dict as one array of bit patterns."""
    parts = []
    for key in sorted(out):
        v = out[key]
        if isinstance(v, dict):
            parts += [bits(v[k]).ravel() for k in sorted(v)]
        elif isinstance(v, np.ndarray):
            parts.append(bits(v).ravel())              # (the integers are exact in a double)
        elif isinstance(v, (int, float)):
            parts.append(bits([float(v)]))
    return np.concatenate(parts)


def test_repeatable_whatever_is_requested_and_after_the_workspace_grew(engine):
    rows = [_abi.SUM_RANGE, EXTRA]
    fac, summ, extra, mask = make_inputs(3001, 3, rows, seed=12)
    kw = dict(classes=16, cells=8, shifts=7, seed=5)
    a = run(engine, fac, summ, extra, mask, rows, **kw)
    b = run(engine, fac, summ, extra, mask, rows, **kw)
    assert np.array_equal(flat(a), flat(b))
    bare = run(engine, fac, summ, extra, mask, rows, want_tables=False, want_null=False, want_curves=False, **kw)
    assert not {"tables", "null_values", "class_stats"} & set(bare)
    for key in bare:
        if isinstance(bare[key], dict):
            for k in bare[key]:
                assert same_bits(bare[key][k], a[key][k]), (key, k)
        elif isinstance(bare[key], np.ndarray):
            assert same_bits(bare[key], a[key]), key
    big = make_inputs(40001, 5, rows, seed=13)
    run(engine, *big, rows, classes=64, cells=64, shifts=9, seed=1)          # a larger call grows the workspace
    c = run(engine, fac, summ, extra, mask, rows, **kw)
    assert np.array_equal(flat(a), flat(c))


# ---------------------------------------------------------------------------------- the Python layer
def test_ishigami_ranking_through_the_analysis_layer(engine):
    """n = 16 384, the factors as a device tensor: the ranking by the excess of delta is x2, x1, x3, dummy; x3 has eta2 about
    0 and a delta clearly above its band; the numbers are those of the yardstick."""
    x, y = ref.ishigami_case()
    summ = np.zeros((_abi.SUMMARY_DIM, x.shape[1]))
    summ[_abi.SUM_APOGEE_ALT] = 1000.0      # passes the outlier filter
    summ[_abi.SUM_RANGE] = 1000.0
    summ[_abi.SUM_FLIGHT_TIME] = 100.0
    summ[_abi.SUM_MAX_SPEED] = y
    names = ["x1", "x2", "x3", "dummy"]
    out = analysis.given_data_sensitivity(dev(engine, summ), dev(engine, x), names, engine=engine, rows=[_abi.SUM_MAX_SPEED])
    d = out["delta"]
    print(f"delta {d['estimate'][0]}, null_hi {d['null_hi'][0]}, excess {d['excess'][0]}, p {d['p_value'][0]}, eta2_adj "
          f"{out['eta2_adj'][0]}")
    assert out["ranking"] == [["x2", "x1", "x3", "dummy"]] and out["row_names"] == ["max_speed"]
    assert out["factor_names"] == names and out["n_samples"] == 16384 and out["count"] == 16384
    want = ref.dependence(x, y[None, :])
    assert same_bits(d["estimate"], want["delta"]["estimate"]) and same_bits(d["null_hi"], want["delta"]["null_hi"])
    assert np.array_equal(d["p_value"], (want["delta"]["exceed"] + 1.0) / 201.0)
    assert np.array_equal(d["excess"], np.maximum(0.0, d["estimate"] - d["null_mean"]))
    assert abs(out["eta2_adj"][0, 2]) < 0.05 and d["estimate"][0, 2] - d["null_hi"][0, 2] >= 0.03
    c = out["curves"][0]["x2"]
    assert len(c["x"]) == 16 and np.all(np.diff(c["x"]) > 0) and c["count"].sum() == 16384
    assert np.array_equal(c["mean"], out["class_stats"][0, 1, :, 1])


def test_a_real_run_through_the_analyzer(engine):
    """run_monte_carlo_device(keep_factors=True), then MonteCarloAnalyzer.given_data_sensitivity: every constant factor (the
    position rows, default sigma 0) has delta = 0 exactly; the population is the one of `drivers`."""
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    an = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    run_out = an.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, precision="f64_fast", keep_factors=True)
    g = an.given_data_sensitivity(run_out, shifts=20)
    d = an.drivers(run_out)
    names = g["factor_names"]
    assert names == list(run_out["factor_names"]) and g["row_names"] == ["apogee_altitude", "range", "flight_time"]
    assert g["count"] == d["count"] and g["n_samples"] == d["n_samples"] and g["n_outliers"] == d["n_outliers"]
    for f, name in enumerate(names):
        if name.startswith("position_"):
            assert np.all(g["delta"]["estimate"][:, f] == 0.0) and np.all(g["delta_num"][:, f] == 0), name
            assert np.all(g["classes_used"][:, f] == 1), name
        else:
            assert np.all(g["classes_used"][:, f] == 16), name
    print(f"apogee: ranking {g['ranking'][0][:5]}, delta excess {np.sort(g['delta']['excess'][0])[::-1][:5]}")
    for j in range(3):
        assert g["delta"]["excess"][j, names.index(g["ranking"][j][0])] > 0.0
