"""tests/casualty_ref.py, the NumPy restatement of erpl_mc_casualty, held to closed forms (no GPU, no library): a uniform
population gives Ec = rho0 sum_k p_k sum_f c_f; one Gaussian group under a uniform population on a fine raster gives
mix_mass = 1 and ec_smooth = ec (the midpoint rule integrates a Gaussian whose bandwidth is two cells to about
2 exp(-2 pi^2 4) = 1e-34); with cells of one bandwidth the deviation is printed next to the 2 exp(-2 pi^2) = 5e-9 of the theory."""
import numpy as np
import pytest

import casualty_ref as ref


def matrix(K, F, m, rng, lo=-80.0, hi=80.0):
    v = np.zeros((5, K * F, m))
    v[0], v[1] = rng.uniform(lo, hi, size=(K * F, m)), rng.uniform(lo, hi, size=(K * F, m))
    v[4] = 50.0
    return v


def test_uniform_population_gives_the_closed_form():
    rng = np.random.default_rng(0)
    K, F, m, rho0 = 5, 3, 200, 3.5e-4
    frags = [(4.0, 0.5, 1.0), (1.0, 7.0, 60.0), (12.0, 0.1, 0.3)]
    p = np.array([0.01, 0.0, 0.02, 0.005, 0.03])
    out = ref.casualty(matrix(K, F, m, rng), m, None, frags, p, np.full((7, 9), rho0), ((-100.0, 100.0), (-100.0, 100.0)), smooth=False)
    want = rho0 * sum(p[k] * sum(f[0] * f[1] for f in frags) for k in range(K))
    assert out["landed"] == out["lethal"] == K * F * m and out["off_grid"] == 0 and out["missing"] == 0 and out["m_c"] == m
    assert abs(out["ec"] - want) <= 1e-14 * want
    assert out["ec_se"] <= 1e-16 * want and out["ec_max_col"] == 0     # every column the same bits
    quantum = out["lethal"] * out["w_max"] * 2.0 ** -out["q"] * rho0 / m
    print(f"ec {out['ec']:.17g}, closed form {want:.17g}, ec_map - ec {out['ec_map'] - out['ec']:.3g}, bound {quantum:.3g}")
    assert abs(out["ec_map"] - out["ec"]) <= quantum + 1e-13 * want
    assert abs((p * out["per_node"]["ec"]).sum() - out["ec"]) <= 1e-14 * want
    assert abs(out["per_fragment"]["ec"].sum() - out["ec"]) <= 1e-14 * want
    assert out["hazard_words"].sum() == (ref.weights(p, [f[0] * f[1] for f in frags], m)[3].sum() * m)
    # a mask and missing jobs: the denominator stays the number of counted columns
    v = matrix(K, F, m, rng)
    v[0, 4, ::2] = np.nan
    mask = np.zeros(m, dtype=np.uint8)
    mask[:50] = 1
    out = ref.casualty(v, m, mask, frags, p, np.full((7, 9), rho0), ((-100.0, 100.0), (-100.0, 100.0)), smooth=False)
    lost = p[1] * frags[1][0] * frags[1][1] * rho0 * 0.5              # row 4 = (node 1, fragment 1): half of its jobs missing
    assert out["m_c"] == 150 and out["missing"] == 75 and np.isnan(out["ec_traj"][:50]).all()
    assert abs(out["ec"] - (want - lost)) <= 1e-13 * want


def gaussian_case(cells_per_bandwidth):
    """One group of one member at the centre of a raster that reaches 9 bandwidths beyond it: H = h_floor^2 I."""
    h = 8.0
    half = 9.0 * h + 0.5 * h / cells_per_bandwidth
    bins = int(round(2.0 * half / (h / cells_per_bandwidth)))
    v = np.zeros((5, 1, 1))
    v[4] = 30.0
    rho0 = 2e-3
    return ref.casualty(v, 1, None, [(3.0, 2.0, 1.0)], [0.25], np.full((bins, bins), rho0), ((-half, half), (-half, half)),
                        h_floor=h, levels=(1e-4,)), 0.25 * 6.0 * rho0


def test_one_gaussian_group_on_a_fine_raster_integrates_to_one():
    out, want = gaussian_case(2)
    assert out["lethal"] == 1 and abs(out["ec"] - want) <= 1e-15 * want
    np.testing.assert_allclose(out["groups"][0, 2:7], [0.0, 0.0, 64.0, 0.0, 64.0])
    print(f"cells of half a bandwidth: mix_mass - 1 = {out['mix_mass'] - 1.0:.3g}, ec_smooth / ec - 1 = {out['ec_smooth'] / out['ec'] - 1.0:.3g}")
    assert abs(out["mix_mass"] - 1.0) <= 1e-12 and abs(out["ec_smooth"] - out["ec"]) <= 1e-12 * out["ec"]
    peak = 0.25 * 6.0 / (2.0 * np.pi * 64.0)
    assert abs(out["risk_smooth"].max() - peak) <= 1e-12 * peak   # an odd number of cells: the member sits on a centre
    assert out["level_area_smooth"][0] > 0.0 and out["level_area"][0] == out["cell_area"]


def test_cells_of_one_bandwidth_print_the_deviation_of_the_midpoint_rule():
    out, want = gaussian_case(1)
    dev = out["mix_mass"] - 1.0
    print(f"cells of one bandwidth: mix_mass - 1 = {dev:.3g} (theory: about 2 exp(-2 pi^2) = {2.0 * np.exp(-2.0 * np.pi ** 2):.3g} per axis)")
    assert abs(dev) <= 1e-7 and abs(out["ec_smooth"] / want - 1.0) <= 1e-7


def test_bins_edges_and_slices():
    e = ref.edges(-3.0, 7.0, 7)
    assert list(ref.bin_of(e, -3.0, 7.0, 7)) == [0, 1, 2, 3, 4, 5, 6, 6]          # the last edge closes the last bin
    x = np.random.default_rng(2).uniform(-3.0, 7.0, 5000)
    assert np.array_equal(ref.bin_of(x, -3.0, 7.0, 7), np.clip(np.searchsorted(e, x, side="right") - 1, 0, 6))
    assert np.array_equal(np.bincount(ref.bin_of(x, -3.0, 7.0, 7), minlength=7), np.histogram(x, bins=7, range=(-3.0, 7.0))[0])
    assert ref.q_of(8192, 16, 8) == 40 and ref.q_of(2 ** 31 - 1, 4096, 1) == 19 and ref.slices(128, 65536) == (16, 8)
    w, w_max, Q, W = ref.weights([0.5, 0.25], [2.0, 0.0], 100)
    assert w_max == 1.0 and Q == 40 and W.tolist() == [[2 ** 40, 0], [2 ** 39, 0]]
    assert ref.weights([0.0], [1.0], 5)[3].tolist() == [[0]]
