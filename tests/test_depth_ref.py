"""The NumPy restatement of erpl_mc_corridor_depth (tests/depth_ref.py) against the definitions themselves, without a GPU:
the pair counts against an enumeration of the pairs, the outliergram identity, the demonstration that a shape outlier hides
inside the pointwise band, and the median flight inside the central region."""
import numpy as np
import pytest

import depth_ref as R
from erpl_monte_carlo_sim_amd import analysis


def _small_table(seed, C=2, T=4, m=9):
    rng = np.random.default_rng(seed)
    v = rng.integers(-2, 3, size=(C, T, m)).astype(np.float64)   # heavy ties
    v[v == 0.0] = np.where(rng.random(np.count_nonzero(v == 0.0)) < 0.5, -0.0, 0.0)
    v[rng.random(v.shape) < 0.1] = np.nan
    v[rng.random(v.shape) < 0.05] = np.inf
    v[rng.random(v.shape) < 0.05] = -np.inf
    mask = (rng.random(m) < 0.2).astype(np.uint8)
    return v, mask


@pytest.mark.parametrize("seed", range(12))
def test_restatement_against_the_enumeration_of_pairs(seed):
    v, mask = _small_table(seed)
    C, T, m = v.shape
    r = R.reference(v, mask)
    assert r["n_masked"] == int(mask.sum())
    for c in range(C):
        sd, sm, nodes = np.zeros(m), np.zeros(m), np.zeros(m, int)
        for k in range(T):
            members = [j for j in range(m) if mask[j] == 0 and np.isfinite(v[c, k, j])]
            assert r["count"][c, k] == len(members)
            n = len(members)
            if n < 2:
                continue
            xs = [v[c, k, j] for j in members]
            for i, j in enumerate(members):
                below = sum(x < xs[i] for x in xs)
                sd[j] += R.brute_pairs(xs, i) / (n * (n - 1) // 2)
                sm[j] += (n - below) / n
                nodes[j] += 1
        assert np.array_equal(r["nodes"][c], nodes)
        d = nodes > 0
        assert np.array_equal(r["depth"][c][d], sd[d] / nodes[d]) and np.all(np.isnan(r["depth"][c][~d]))
        assert np.array_equal(r["mei"][c][d], sm[d] / nodes[d]) and np.all(np.isnan(r["mei"][c][~d]))
        # sentence 4 by a plain sort
        nd = int(d.sum())
        assert r["n_defined"][c] == nd
        if nd == 0:
            assert r["median"][c] == -1 and np.isnan(r["threshold"][c]) and r["n_central"][c] == 0
            continue
        order = sorted(r["depth"][c][d], reverse=True)
        h = min(max(int(np.ceil(0.5 * nd)), 1), nd)
        assert r["threshold"][c] == order[h - 1] and r["depth_max"][c] == order[0]
        s = d & (np.nan_to_num(r["depth"][c], nan=-1.0) >= order[h - 1])
        assert np.array_equal(r["central"][c].astype(bool), s) and r["n_central"][c] == s.sum() >= h
        assert r["median"][c] == min(j for j in range(m) if d[j] and r["depth"][c][j] == order[0])
        for k in range(T):
            members = [j for j in range(m) if mask[j] == 0 and np.isfinite(v[c, k, j])]
            cen = [v[c, k, j] for j in members if s[j]]
            assert r["n_central_here"][c, k] == len(cen)
            if cen:
                lo, hi = min(cen), max(cen)
                assert r["central_lo"][c, k] == lo and r["central_hi"][c, k] == hi
                assert r["fence_lo"][c, k] == lo - 1.5 * (hi - lo) and r["fence_hi"][c, k] == hi + 1.5 * (hi - lo)
            else:
                assert all(np.isnan(r[f][c, k]) for f in ("central_lo", "central_hi", "fence_lo", "fence_hi"))
        for j in range(m):
            out = [k for k in range(T) if mask[j] == 0 and np.isfinite(v[c, k, j]) and np.isfinite(r["fence_lo"][c, k])
                   and np.isfinite(r["fence_hi"][c, k]) and (v[c, k, j] < r["fence_lo"][c, k] or v[c, k, j] > r["fence_hi"][c, k])]
            assert r["n_out"][c, j] == len(out) and r["first_out"][c, j] == (out[0] if out else -1)
        assert r["n_outliers"][c] == sum(1 for j in range(m) if d[j] and r["n_out"][c, j] > 0)
        for k in range(T):
            keep = [v[c, k, j] for j in range(m) if mask[j] == 0 and np.isfinite(v[c, k, j]) and d[j] and r["n_out"][c, j] == 0]
            if keep:
                assert r["whisker_lo"][c, k] == min(keep) and r["whisker_hi"][c, k] == max(keep)
            else:
                assert np.isnan(r["whisker_lo"][c, k]) and np.isnan(r["whisker_hi"][c, k])


def test_outliergram_identity_on_curves_that_never_cross():
    v = R.demo_curves()
    t = (np.arange(v.shape[1]) + 0.5) / v.shape[1]
    v[0, :, 0] = 1.01 * np.sin(np.pi * t)   # the shape outlier replaced by one more multiple of the same curve
    r = R.reference(v)
    n = v.shape[2]
    assert np.all(r["nodes"][0] == v.shape[1]) and np.all(r["count"] == n)
    d = R.outliergram_distance(r["depth"][0], r["mei"][0], n)
    assert np.max(np.abs(d)) <= 1e-12, np.max(np.abs(d))
    d2, flags = analysis.outliergram(r["depth"][0], r["mei"][0], n)
    assert np.array_equal(d, d2) and not flags.any()


def test_a_shape_outlier_hides_inside_the_pointwise_band():
    v = R.demo_curves()
    x = v[0]
    lo, hi = np.quantile(x, (0.05, 0.95), axis=1)
    assert np.all((x[:, 0] >= lo) & (x[:, 0] <= hi)), "the shape outlier lies inside the 5 - 95 % band at every node"
    r = R.reference(v)
    d, flags = analysis.outliergram(r["depth"][0], r["mei"][0], x.shape[1])
    print("outliergram distance of the shape outlier", d[0], "largest of the others", np.abs(d[1:]).max())
    assert list(np.flatnonzero(flags)) == [0], "it is the only flag"
    assert d[0] > 1e3 * np.abs(d[1:]).max()
    # the 1.6-amplitude curve is a magnitude outlier, and the shape outlier is not
    assert r["n_out"][0, 1] == x.shape[0] and r["first_out"][0, 1] == 0 and r["n_out"][0, 0] == 0
    assert r["n_outliers"][0] == 1


@pytest.mark.parametrize("seed", range(4))
def test_the_median_column_lies_inside_the_central_region(seed):
    v, mask = R.make_case(2, 9, 257, 260, seed=seed)
    r = R.reference(v, mask, m=257)
    for c in range(2):
        j = int(r["median"][c])
        assert j >= 0 and mask[j] == 0 and r["central"][c, j] == 1
        for k in range(9):
            if np.isfinite(v[c, k, j]):
                assert r["central_lo"][c, k] <= v[c, k, j] <= r["central_hi"][c, k]
