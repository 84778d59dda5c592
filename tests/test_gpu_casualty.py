"""erpl_mc_casualty on the device against tests/casualty_ref.py, on synthetic matrices built with torch (no flights but in the
last test).  Shapes are the smallest at which the kernels can go wrong: m on both sides of a wave, of a workgroup and of the
1024-member tile of the smoothing pass, ld > m, masked and NaN columns interleaved, groups of 0, 1, 2 and 3 members, rasters
1 x 1, 3 x 5 and 64 x 48.

What is held, per case:
  1. bit for bit: ec_traj (NaN pattern included), the int64 map, every count, ec_max with its column, the level areas of the counts
  2. to 1e-12 relative, the bound of the project's fixed-order folds: ec, ec_std, ec_se, ec_node, ec_fragment, S_kf, the group
     means and H; sum_k p_fail[k] ec_node[k] = sum_f ec_fragment[f] = ec; ec_map within lethal * w_max * 2^-Q * max(pop) / m_c
  3. risk_smooth by the measured-tolerance rule of tests/test_gpu_density.py, restated here for a mixture: truth is the mixture in
     np.longdouble with the H the call returned; the direct and the whitened float64 formulations are measured against it; body
     (>= 1e-12 of the peak) and tail (>= 1e-280) nodes within 4 x the worse of the two plus (members + 64 rows) 2^-53, dead
     nodes <= 1e-279 x peak, every node in a class
  4. two calls the same bytes; a permutation of the columns (mask alike) the same map bytes and counts; sentinels untouched"""
import ctypes as C

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import casualty_ref as ref
import helpers as H
from test_casualty_abi import check_refusals

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
RANGES = ((-400.0, 1100.0), (-300.0, 900.0))
SENTINEL = 777.25


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng


def fragments_of(F):
    return [(1.0 + (f % 3), 0.25 * (1 + f % 4), 0.2 + 3.0 * f) for f in range(F)]


def p_fail_of(K):
    p = 0.5 * (1.0 + np.arange(K)) / (1.0 + np.arange(K)).sum()
    if K > 2:
        p[1] = 0.0
    return p


def population_of(bins, seed=3):
    rng = np.random.default_rng(seed)
    pop = 1e-4 * (0.5 + rng.random(bins))
    pop.reshape(-1)[::7] = 0.0
    return pop


def synthetic(m, ld, K, F, seed, kind="cloud"):
    """values [5, K F, ld] and the mask [m] as NumPy: correlated clouds off the origin, one centre per row, some beyond the
    raster; every 7th column of a row NaN in one of the three channels, every 5th column masked; rows 0..3 keep 0, 1, 2 and 3
    members; the columns beyond m hold a finite sentinel that would count if it were read."""
    rng = np.random.default_rng(seed)
    R = K * F
    v = np.full((5, R, ld), SENTINEL)
    for r in range(R):
        cx, cy = 250.0 + 37.0 * (r % 11), 200.0 + 23.0 * (r % 7)
        a, b = rng.normal(size=m), rng.normal(size=m)
        v[0, r, :m] = cx + 180.0 * a
        v[1, r, :m] = cy + 90.0 * a + 120.0 * b
        v[4, r, :m] = 60.0 * rng.random(m)
        v[2, r, :m], v[3, r, :m] = rng.random(m), rng.random(m)
        bad = np.arange(m) % 7 == (r % 7)
        v[(0, 1, 4)[r % 3], r, :m][bad] = (np.nan, np.inf, -np.inf)[r % 3]
    if kind == "one-cell":
        v[0, :, :m] = np.where(np.isfinite(v[0, :, :m]), 333.0, v[0, :, :m])
        v[1, :, :m] = np.where(np.isfinite(v[1, :, :m]), 444.0, v[1, :, :m])
    if kind == "edges":
        ex, ey = ref.edges(*RANGES[0], 3), ref.edges(*RANGES[1], 5)
        pts_x = np.concatenate([ex, [np.nextafter(ex[0], -np.inf), np.nextafter(ex[-1], np.inf), 5000.0, -5000.0]])
        pts_y = np.concatenate([ey, [np.nextafter(ey[0], -np.inf), np.nextafter(ey[-1], np.inf), 0.0, 0.0]])
        for r in range(R):
            j = np.arange(m)
            v[0, r, :m] = pts_x[(j + r) % len(pts_x)]
            v[1, r, :m] = pts_y[(j // 3 + 2 * r) % len(pts_y)]
    if R >= 4 and m >= 8:
        live = np.flatnonzero(np.arange(m) % 5 != 0)
        for r, keep in enumerate((0, 1, 2, 3)):
            v[0, r, :m] = np.nan
            if kind == "cloud":
                v[0, r, live[:keep] if keep else []] = 300.0 + 50.0 * np.arange(keep)
                v[4, r, live[:keep] if keep else []] = 100.0
                v[1, r, live[:keep] if keep else []] = 250.0 - 20.0 * np.arange(keep) ** 2
    mask = (np.arange(m) % 5 == 0).astype(np.uint8) * 3 if m > 1 else None
    return v, mask


# (label, m, ld, (K, F), raster, kind, ke_min, p_fail of zeros)
CASES = [("m1", 1, 3, (1, 1), (1, 1), "cloud", 15.0, False), ("m63", 63, 70, (3, 5), (3, 5), "cloud", 15.0, False),
         ("m64", 64, 65, (1, 1), (64, 48), "cloud", 0.0, False), ("m65", 65, 80, (16, 8), (64, 48), "cloud", 15.0, False),
         ("m255", 255, 256, (3, 5), (64, 48), "cloud", 15.0, False), ("m256", 256, 300, (16, 8), (3, 5), "cloud", 15.0, False),
         ("m257", 257, 260, (3, 5), (1, 1), "cloud", 15.0, False), ("m1025", 1025, 1030, (1, 1), (64, 48), "cloud", 15.0, False),
         ("m1025-rows", 1025, 1100, (3, 5), (3, 5), "cloud", 15.0, False),
         ("one-cell", 257, 300, (3, 5), (64, 48), "one-cell", 15.0, False), ("edges", 65, 66, (3, 5), (3, 5), "edges", 0.0, False),
         ("ke-cut", 257, 258, (3, 5), (3, 5), "cloud", 2500.0, False), ("p-zero", 65, 70, (3, 5), (3, 5), "cloud", 15.0, True)]


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = np.isnan(b) | (np.abs(a - b) <= rel * np.abs(b))
    assert ok.all(), (a[~ok], b[~ok])


def judge_mixture(label, got, want, out, values, m, mask, frags, raster, ranges):
    """The measured-tolerance rule for the mixture the call evaluated: the members by the restatement, H as the call returned it."""
    assert np.finfo(LD).nmant == 63   # x86-64 extended precision: a long double that is a double would be no truth
    K_F = out["groups"].shape[0]
    F = len(frags)
    gx, gy = ref.centres(*ranges[0], raster[0]), ref.centres(*ranges[1], raster[1])
    QX, QY = np.repeat(gx, raster[1]), np.tile(gy, raster[0])
    counted = np.ones(m, dtype=bool) if mask is None else mask == 0
    t, direct, white = np.zeros(len(QX), dtype=LD), np.zeros(len(QX)), np.zeros(len(QX))
    members = rows = 0
    for r in range(K_F):
        x, y, v = values[0, r, :m], values[1, r, :m], values[4, r, :m]
        with np.errstate(invalid="ignore", over="ignore"):
            sel = counted & np.isfinite(x) & np.isfinite(y) & np.isfinite(v) & ((0.5 * frags[r % F][2]) * (v * v) >= want["ke_min"])
        if not sel.any():
            continue
        g = out["groups"][r]
        assert int(g[0]) == int(sel.sum())
        Hm, weight = (g[4], g[5], g[6]), g[7] / out["m_c"]
        t += ref.mixture_term(QX, QY, x[sel], y[sel], Hm, weight, dtype=LD)
        direct += ref.mixture_term(QX, QY, x[sel], y[sel], Hm, weight)
        white += ref.mixture_term_whitened(QX, QY, x[sel], y[sel], Hm, weight)
        members += int(sel.sum())
        rows += 1
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    assert np.isfinite(got).all() and (got >= 0.0).all()
    peak = t.max()
    if not peak > 0:
        assert not got.any()
        print(f"{label}: an empty mixture, all zeros")
        return
    ratio = t / peak
    classes = (("body", ratio >= LD(1e-12)), ("tail", (ratio >= LD(1e-280)) & (ratio < LD(1e-12))), ("dead", ratio < LD(1e-280)))
    assert sum(int(s.sum()) for _, s in classes) == len(t)   # no node is left out
    for name, s in classes:
        if not s.any():
            continue
        if name == "dead":
            worst = float(got[s].max() / float(peak))
            print(f"{label} dead: {int(s.sum())} nodes, device max / peak {worst:.3g}")
            assert worst <= 1e-279
            continue
        rel = lambda v: float((np.abs(v[s].astype(LD) - t[s]) / t[s]).max())   # noqa: E731
        e_dev, e_ref = rel(got), [rel(direct), rel(white)]
        bound = 4.0 * max(e_ref) + (members + 64 * rows) * U
        print(f"{label} {name}: {int(s.sum())} nodes, device {e_dev:.3g}, direct {e_ref[0]:.3g}, whitened {e_ref[1]:.3g}, bound {bound:.3g}")
        assert e_dev <= bound, (label, name, e_dev, e_ref, bound)


def compare(label, out, want, values, m, mask, frags, p_fail, raster, pop, ranges=RANGES):
    # 1. bit for bit
    ec = out["ec_traj"].cpu().numpy()
    assert ec.shape == (m,) and np.array_equal(ec.view(np.int64), want["ec_traj"].view(np.int64)), label
    assert np.array_equal(out["hazard_words"], want["hazard_words"]) and out["hazard_words"].dtype == np.int64
    for k in ("m_c", "landed", "lethal", "off_grid", "missing", "q", "ec_max_col"):
        assert out[k] == want[k], (label, k, out[k], want[k])
    assert out["ec_max"] == want["ec_max"] or (np.isnan(out["ec_max"]) and np.isnan(want["ec_max"]))
    assert out["level_area"] == want["level_area"] and out["w_max"] == want["w_max"] and out["cell_area"] == want["cell_area"]
    assert np.array_equal(out["hazard"], want["hazard"])
    for split in ("per_node", "per_fragment"):
        for k in analysis.CASUALTY_COUNTS:
            assert np.array_equal(out[split][k], want[split][k]), (label, split, k)
    assert np.array_equal(out["groups"][:, 0], want["groups"][:, 0]) and np.array_equal(out["groups"][:, 7], want["groups"][:, 7])
    # 2. to 1e-12
    for k in ("ec", "ec_std", "ec_se"):
        close(out[k], want[k])
    close(out["per_node"]["ec"], want["per_node"]["ec"])
    close(out["per_fragment"]["ec"], want["per_fragment"]["ec"])
    close(out["groups"][:, 1:7], want["groups"][:, 1:7])
    if out["m_c"]:
        close(float((p_fail * out["per_node"]["ec"]).sum()), out["ec"])
        close(float(out["per_fragment"]["ec"].sum()), out["ec"])
        quantum = out["lethal"] * out["w_max"] * 2.0 ** -out["q"] * pop.max() / out["m_c"]
        print(f"{label}: ec {out['ec']:.6g}, ec_map - ec {out['ec_map'] - out['ec']:.3g}, bound {quantum:.3g}; missing {out['missing']}, "
              f"off the raster {out['off_grid']}")
        assert abs(out["ec_map"] - out["ec"]) <= quantum + 1e-12 * out["ec"]
    close(out["ec_map"], want["ec_map"])
    # 3. the smoothed map
    judge_mixture(label, out["risk_smooth"], want, out, values, m, mask, frags, raster, ranges)
    risk = out["risk_smooth"].reshape(-1)
    close(out["ec_smooth"], float(((risk * pop.reshape(-1)) * out["cell_area"]).sum()))
    assert out["level_area_smooth"] == [float((risk >= lv).sum()) * out["cell_area"] for lv in out["levels"]]
    denom = float(((out["groups"][:, 7] * out["groups"][:, 0]) / out["m_c"]).sum()) if out["m_c"] else 0.0
    if denom > 0.0:
        close(out["mix_mass"], float((risk * out["cell_area"]).sum() / denom))
        print(f"{label}: ec_smooth {out['ec_smooth']:.6g}, mix_mass {out['mix_mass']:.6g}")
    else:
        assert np.isnan(out["mix_mass"])


@pytest.mark.parametrize("label,m,ld,shape,raster,kind,ke_min,pzero", CASES, ids=[c[0] for c in CASES])
def test_casualty_equals_the_restatement(engine, label, m, ld, shape, raster, kind, ke_min, pzero):
    K, F = shape
    values, mask = synthetic(m, ld, K, F, 100 + m + K, kind)
    frags, pop = fragments_of(F), population_of(raster)
    p_fail = np.zeros(K) if pzero else p_fail_of(K)
    levels = (1e-9, 1e-7, 1e-6)
    want = ref.casualty(values, m, mask, frags, p_fail, pop, RANGES, ke_min=ke_min, levels=levels, want_risk=False)
    want["ke_min"] = ke_min
    dv, dm = torch.as_tensor(values, device=engine.device), None if mask is None else torch.as_tensor(mask, device=engine.device)
    dp = torch.as_tensor(pop, device=engine.device)
    before = dv.clone()
    out = engine.casualty(dv, frags, p_fail, dp, RANGES, mask=dm, m=m, ke_min=ke_min, levels=levels)
    assert torch.equal(dv.view(torch.int64), before.view(torch.int64))          # the matrix, its sentinels included, is read only
    compare(label, out, want, values, m, mask, frags, p_fail, raster, pop)
    groups = want["groups"][:, 0]
    if label == "m65":
        assert list(groups[:4]) == [0.0, 1.0, 2.0, 3.0]                         # groups of 0, 1, 2 and 3 members
    if label == "one-cell":
        assert np.count_nonzero(out["hazard_words"]) == 1
    if label == "edges":
        assert out["off_grid"] > 0 and np.count_nonzero(out["hazard_words"]) > 1
    if label == "ke-cut":
        assert 0 < out["lethal"] < out["landed"]
    if pzero:
        assert out["ec"] == 0.0 and out["ec_std"] == 0.0 and not out["hazard_words"].any() and not out["risk_smooth"].any()
    # 4. a second call: the same bytes
    again = engine.casualty(dv, frags, p_fail, dp, RANGES, mask=dm, m=m, ke_min=ke_min, levels=levels)
    for k in ("risk_smooth", "hazard", "hazard_words", "groups"):
        assert np.array_equal(out[k].view(np.int64), again[k].view(np.int64)), (label, k)
    assert torch.equal(out["ec_traj"].view(torch.int64), again["ec_traj"].view(torch.int64))
    for k in ("ec", "ec_std", "ec_smooth", "mix_mass", "ec_map"):
        assert np.float64(out[k]).view(np.int64) == np.float64(again[k]).view(np.int64), (label, k)


def test_a_permutation_of_the_columns_leaves_the_map_and_the_counts(engine):
    m, ld, K, F = 257, 257, 3, 5
    values, mask = synthetic(m, ld, K, F, 9)
    frags, pop, p_fail = fragments_of(F), population_of((64, 48)), p_fail_of(K)
    perm = np.random.default_rng(1).permutation(m)
    dp = torch.as_tensor(pop, device=engine.device)
    run = lambda v, k: engine.casualty(torch.as_tensor(np.ascontiguousarray(v), device=engine.device), frags, p_fail, dp, RANGES,   # noqa: E731
                                       mask=torch.as_tensor(np.ascontiguousarray(k), device=engine.device), smooth=False)
    a, b = run(values, mask), run(values[:, :, perm], mask[perm])
    assert a["hazard_words"].tobytes() == b["hazard_words"].tobytes() and a["hazard_words"].any()
    for k in ("m_c", "landed", "lethal", "off_grid", "missing"):
        assert a[k] == b[k]
    for split in ("per_node", "per_fragment"):
        for k in analysis.CASUALTY_COUNTS:
            assert np.array_equal(a[split][k], b[split][k])
    assert np.array_equal(a["ec_traj"].cpu().numpy()[perm].view(np.int64), b["ec_traj"].cpu().numpy().view(np.int64))
    assert a["risk_smooth"] is None and np.isnan(a["ec_smooth"]) and np.isnan(a["mix_mass"])
    assert np.isnan(a["groups"][:, 2:7]).all() and np.array_equal(a["groups"][:, 0], b["groups"][:, 0])


def test_sentinels_and_refusals_through_the_c_abi(engine):
    lib = engine.lib
    check_refusals(lib)                                               # the order of the header, each with its message
    m, ld, K, F, raster = 65, 80, 3, 5, (3, 5)
    values, mask = synthetic(m, ld, K, F, 11)
    frags, pop, p_fail = fragments_of(F), population_of(raster), p_fail_of(K)
    spec = analysis.casualty_spec(K, frags, raster, RANGES, smooth=False)
    dv, dm = torch.as_tensor(values, device=engine.device), torch.as_tensor(mask, device=engine.device)
    dp = torch.as_tensor(pop, device=engine.device)
    ec = torch.full((m + 16,), SENTINEL, dtype=torch.float64, device=engine.device)
    risk, hazard = np.full(raster, SENTINEL), np.full(raster, SENTINEL)
    res = _abi.ErplCasualty()
    st = torch.cuda.current_stream(engine.device)

    def call(population, ec_t, hz):
        return lib.erpl_mc_casualty(engine._ctx, C.c_void_p(dv.data_ptr()), ld, m, C.c_void_p(dm.data_ptr()), C.byref(spec),
                                    C.c_void_p(p_fail.ctypes.data), C.c_void_p(population.data_ptr()), C.c_void_p(ec_t.data_ptr()), None,
                                    None, None, C.c_void_p(hz.ctypes.data), None, C.c_void_p(risk.ctypes.data), C.byref(res),
                                    C.c_void_p(st.cuda_stream))

    # a population entry that is negative or not finite: refused after the first pass, nothing written
    for bad in (-1e-300, float("nan"), float("inf")):
        worse = dp.clone()
        worse[2, 3] = bad
        assert call(worse, ec, hazard) == -1 and "population" in lib.erpl_mc_last_error().decode()
        assert bool((ec == SENTINEL).all()) and (hazard == SENTINEL).all() and (risk == SENTINEL).all()
    assert call(dp, ec, hazard) == 0
    got = ec.cpu().numpy()
    assert (got[m:] == SENTINEL).all() and not (got[:m] == SENTINEL).any()   # beyond column m: untouched
    assert (risk == SENTINEL).all() and not (hazard == SENTINEL).any()        # smooth = 0: the smoothed map is not written
    want = ref.casualty(values, m, mask, frags, p_fail, pop, RANGES, smooth=False)
    assert np.array_equal(got[:m].view(np.int64), want["ec_traj"].view(np.int64)) and np.array_equal(hazard, want["hazard"])


def test_one_real_run_through_the_python_layers():
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    debris = [(20.0, 10.0), (float("inf"), 0.0)]
    foot = mc.debris_footprint(dict(H.EXAMPLE_IC), 16, fragments=debris, stride=25, nodes=4, seed=5, planar=True, dt=0.25,
                               max_steps=20000)
    vals = foot["values"].cpu().numpy()
    x, y = vals[0][np.isfinite(vals[0])], vals[1][np.isfinite(vals[1])]
    assert len(x) > 0
    ranges = ((x.min() - 50.0, x.max() + 50.0), (y.min() - 50.0, y.max() + 50.0))
    pop = np.full((16, 12), 1e-5)
    pop[8:, :] = 2e-3                                               # a two-level population raster
    frags = [(30.0, 0.3, 0.5), (1.0, 6.0, 80.0)]
    out = mc.casualty_expectation(foot, pop, ranges, fragments=frags, failure_rate=0.002, ke_min=15.0, levels=(1e-6, 1e-5))
    mask = foot["reasons"].cpu().numpy()
    p_fail = analysis.failure_probabilities(foot["time"], 0.002)
    np.testing.assert_array_equal(out["p_fail"], p_fail)
    want = ref.casualty(vals, 16, mask, frags, p_fail, pop, ranges, levels=(1e-6, 1e-5), want_risk=False)
    want["ke_min"] = 15.0
    compare("real", out, want, vals, 16, mask, frags, p_fail, (16, 12), pop, ranges)
    assert out["lethal"] > 0 and out["ec"] > 0.0 and out["time"].shape == (4,) and out["ec_contribution"].shape == (4,)
    ci = mc.confidence_intervals(foot, replicates=200, extra=out["ec_traj"])
    assert ci["extra"]["mean"]["estimate"] == pytest.approx(out["ec"], rel=1e-12) or ci["count"] < out["m_c"]
    assert ci["extra"]["mean"]["se"] >= 0.0 and "apogee_altitude" in ci
    assert mc.plot_casualty(out, save_plots=False) is None
