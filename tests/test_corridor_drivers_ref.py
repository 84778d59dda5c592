"""The NumPy restatement of erpl_mc_corridor_drivers (corridor_drivers_ref.restate, written from include/erpl_mc.h) held row by
row to np.corrcoef and to np.linalg.lstsq on the standardised columns of the row's own population: the yardstick of
tests/test_gpu_corridor_drivers.py pinned without a GPU.  Bounds: np.corrcoef and lstsq are other algorithms on the same
data, so 1e-12 on a correlation and 1e-12 * 10 * cond on a coefficient (src_bound), the bounds the device is held to."""
import numpy as np
import pytest

import corridor_drivers_ref as ref

SHAPES = ((1, 1, 1, 1), (257, 300, 5, 21), (1000, 1024, 19, 130), (4099, 4099, 32, 21))


@pytest.mark.parametrize("m,ld,F,R", SHAPES)
def test_restatement_against_corrcoef_and_lstsq(m, ld, F, R):
    x, y, mask = ref.make_case(m, ld, F, R, seed=11 + m)
    out = ref.restate(x, y, mask, m)
    base = (mask == 0) & np.isfinite(x[:, :m]).all(axis=0)
    assert out["n_base"] == int(base.sum()) and out["n_base"] + out["n_masked"] + out["n_factor_non_finite"] == m
    assert out["n_masked"] == int((mask != 0).sum())
    checked = fitted = 0
    for r in range(R):
        pop = base & np.isfinite(y[r, :m])
        n = int(pop.sum())
        assert out["count"][r] == n
        if n < 2:
            assert np.isnan(out["pearson"][r]).all() and np.isnan(out["src"][r]).all() and not out["regression_ok"][r]
            continue
        xr, yr = x[:, :m][:, pop], y[r, :m][pop]
        assert out["mean"][r] == pytest.approx(yr.mean(), rel=1e-13) and out["std"][r] == pytest.approx(yr.std(), rel=1e-12, abs=1e-300)
        varies = xr.min(axis=1) != xr.max(axis=1)
        if yr.min() == yr.max():
            assert out["constant"][r] and np.isnan(out["pearson"][r]).all() and np.isnan(out["src"][r]).all() and np.isnan(out["r2"][r])
            continue
        with np.errstate(all="ignore"):
            cc = np.corrcoef(np.vstack([xr, yr]))
        assert np.isnan(out["pearson"][r, ~varies]).all()
        assert np.max(np.abs(out["pearson"][r, varies] - cc[F, :F][varies]), initial=0.0) <= 1e-12
        checked += int(varies.sum())
        use = np.flatnonzero(varies)
        if n <= len(use):
            assert not out["regression_ok"][r] and np.isnan(out["src"][r]).all() and not out["pivot_min"][r] >= ref.PIVOT
            continue
        assert out["regression_ok"][r] and out["pivot_min"][r] >= ref.PIVOT
        zx = ((xr[use] - xr[use].mean(axis=1)[:, None]) / xr[use].std(axis=1)[:, None]).T
        zy = (yr - yr.mean()) / yr.std()
        beta, *_ = np.linalg.lstsq(zx, zy, rcond=None)
        bound = ref.src_bound(out["cond"][r])
        assert np.max(np.abs(out["src"][r, use] - beta), initial=0.0) <= bound, (r, out["cond"][r])
        assert np.isnan(out["src"][r, ~varies]).all()
        r2 = 1.0 - np.sum((zy - zx @ beta) ** 2) / np.sum(zy ** 2)
        assert abs(out["r2"][r] - r2) <= bound
        fitted += 1
    if m > 1:
        assert checked > 0 and fitted > 0
        assert not np.isfinite(x[0, 5]) and out["n_factor_non_finite"] >= (mask[5] == 0)
    if F >= 5:   # the rows and factors with a meaning of their own
        assert out["count"][ref.ROW_ALL_NAN] == 0 and np.isnan(out["mean"][ref.ROW_ALL_NAN]) and not out["constant"][ref.ROW_ALL_NAN]
        assert out["count"][ref.ROW_ONE] == 1 and out["constant"][ref.ROW_ONE] and out["mean"][ref.ROW_ONE] == 1.25
        assert out["constant"][ref.ROW_CONSTANT] and out["count"][ref.ROW_CONSTANT] > 2 and out["std"][ref.ROW_CONSTANT] == 0.0
        assert out["constant"][ref.ROW_ZEROS] and out["count"][ref.ROW_ZEROS] > 2
        assert out["factor_constant"].tolist() == [f == 2 for f in range(F)]
        assert np.isnan(out["pearson"][:, 2]).all()
        k = ref.ROW_FACTOR_CONSTANT
        assert out["count"][k] > 2 * F and np.isnan(out["pearson"][k, 3]) and np.isnan(out["src"][k, 3]) and out["regression_ok"][k]
        assert np.isfinite(out["pearson"][0, 3]) and np.isfinite(out["pearson"][k, 0])
        assert out["count"][ref.ROW_COUNT_F] == F - 1 and not out["regression_ok"][ref.ROW_COUNT_F]
        others = [r for r in range(R) if out["count"][r] > 3 * F]
        assert len(others) >= R - 6 and out["regression_ok"][others].all() and (out["cond"][others] <= 10.0).all()


def test_an_affine_pair_fails_every_regression_and_keeps_the_correlations():
    x, y, mask = ref.make_case(257, 300, 5, 21, seed=5, affine=True)
    out = ref.restate(x, y, mask, 257)
    assert not out["regression_ok"].any() and np.isnan(out["src"]).all() and np.isnan(out["r2"]).all()
    assert np.isfinite(out["pearson"][0, [0, 1, 3, 4]]).all()
    assert abs(out["pearson"][0, 4] + out["pearson"][0, 1]) <= 1e-12   # the image runs the other way


def test_without_the_regression_and_without_a_mask():
    x, y, mask = ref.make_case(257, 300, 5, 21, seed=6)
    a, b = ref.restate(x, y, mask, 257), ref.restate(x, y, mask, 257, regression=False)
    assert b["src"] is None and np.isnan(b["r2"]).all() and not b["regression_ok"].any()
    assert np.array_equal(a["pearson"], b["pearson"], equal_nan=True)
    c = ref.restate(x, y, None, 257)
    assert c["n_masked"] == 0 and c["n_base"] == 256 and (c["count"] >= a["count"]).all()
