"""erpl_mc_corridor_depth on a real MI355X (`pytest -m gpu`) against the NumPy restatement of the definitions in
include/erpl_mc.h (depth_ref.reference, itself held to an enumeration of the pairs by test_depth_ref.py).

Bounds.  Everything before the divisions is integer arithmetic and every floating-point operation of the contract is one
IEEE operation, so: every integer output and flag exact; depth, mei, threshold, depth_max and the fences the same BITS;
envelopes and whiskers equal by value (the sign of a zero extreme is not part of the contract, and a fence that is zero
inherits it: lo - factor * 0); NaN exactly where the restatement has NaN."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import depth_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

L = _abi.DEPTH_LDS_MAX
# (C, T, m, ld): one column; two; around a wave; several workgroups' worth of columns; every channel; the LDS boundary; and a
# row longer than a segment of the segmented sort (the global path's device-wide sort per row)
SHAPES = ((1, 1, 1, 1), (1, 2, 2, 2), (2, 5, 63, 64), (2, 5, 64, 64), (2, 5, 65, 80), (3, 21, 1025, 1100), (8, 3, 4099, 4099),
          (1, 3, L, L), (1, 3, L + 1, L + 16), (1, 2, 131073, 131073))
INT_KEYS = ("count", "n_central_here", "n_defined", "n_central", "n_outliers", "median", "nodes", "n_out", "first_out", "central")
BIT_KEYS = ("depth", "mei", "threshold", "depth_max", "fence_lo", "fence_hi")
VALUE_KEYS = ("central_lo", "central_hi", "whisker_lo", "whisker_hi")


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(engine, v, mask=None, m=None, **kw):
    dev = engine.device
    out = engine.corridor_depth(torch.from_numpy(v).to(dev), mask=None if mask is None else torch.from_numpy(mask).to(dev), m=m, **kw)
    return {k: (x.cpu().numpy() if torch.is_tensor(x) else x) for k, x in out.items()}


def hold(got, want, what):
    assert got["m"] == want["m"] and got["n_masked"] == want["n_masked"], what
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in BIT_KEYS:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k, "NaN")
        ok = ~np.isnan(w) & (w != 0.0)   # a zero fence is the zero extreme it was made of: by value, like the extremes
        assert same_bits(g[ok], w[ok]) and np.all(g[w == 0.0] == 0.0), (what, k)
    for k in VALUE_KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)


def identical(a, b, keys=None):
    for k in keys or a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
        else:
            assert x == y, k


@pytest.fixture(scope="module")
def mid_case(engine):
    """(3, 21, 1025, 1100): the input, the restatement and the device's result, shared by the tests that compare paths."""
    v, mask = R.make_case(3, 21, 1025, 1100)
    return v, mask, R.reference(v, mask, 1025), run(engine, v, mask, 1025)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(k) for k in s))
def test_against_the_restatement(engine, shape):
    C, T, m, ld = shape
    v, mask = R.make_case(C, T, m, ld)
    want = R.reference(v, mask, m)
    hold(run(engine, v, mask, m), want, shape)
    if m <= 4099:   # without a mask, and the other path (every shape here fits both)
        hold(run(engine, v, None, m), R.reference(v, None, m), (shape, "no mask"))
        hold(run(engine, v, mask, m, lds_limit=1), want, (shape, "global path"))


def test_special_rows(engine):
    rng = np.random.default_rng(11)
    C, T, m = 3, 6, 300
    v = rng.normal(size=(C, T, m))
    v[0, 1, :] = 2.5                      # a row of one repeated value
    v[0, 2, :] = np.nan
    v[0, 2, 17] = 1.0                     # a row with n = 1
    v[0, 3, :] = np.nan                   # an empty row
    v[1, :, :] = np.nan                   # a channel with no defined column
    v[1, :, 5] = 3.0                      # .. but populations of one
    v[2] = np.round(2.0 * v[2])           # integer-valued data: heavy ties, both zeros
    v[2][v[2] == 0.0] = np.where(rng.random(np.count_nonzero(v[2] == 0.0)) < 0.5, -0.0, 0.0)
    mask = (rng.random(m) < 0.1).astype(np.uint8)
    mask[5] = 0
    want = R.reference(v, mask)
    assert want["n_defined"][1] == 0 and want["median"][1] == -1 and want["count"][0, 2] == 1 and want["count"][0, 3] == 0
    got = run(engine, v, mask)
    hold(got, want, "special rows")
    assert np.isnan(got["threshold"][1]) and np.all(np.isnan(got["depth"][1])) and np.all(got["central"][1] == 0)
    hold(run(engine, v, mask, lds_limit=16), want, "special rows, global path")


def test_central_one_and_factor_zero(engine):
    v, mask = R.make_case(2, 7, 513, 520)
    want = R.reference(v, mask, 513, central=1.0, factor=0.0)
    got = run(engine, v, mask, 513, central=1.0, factor=0.0)
    hold(got, want, "central = 1, factor = 0")
    # every defined column is central, so nothing lies outside the envelope, whatever the factor
    assert np.array_equal(got["n_central"], got["n_defined"]) and np.all(got["n_out"] == 0) and np.all(got["n_outliers"] == 0)
    hold(run(engine, v, mask, 513, central=1.0, factor=1.5), R.reference(v, mask, 513, central=1.0, factor=1.5), "central = 1")
    want0 = R.reference(v, mask, 513, central=0.5, factor=0.0)
    got0 = run(engine, v, mask, 513, central=0.5, factor=0.0)
    hold(got0, want0, "factor = 0")
    assert np.all(got0["n_outliers"] > 0) and same_bits(got0["fence_lo"], got0["central_lo"])


def test_the_global_path_gives_the_bytes_of_the_lds_path(engine, mid_case):
    v, mask, want, got = mid_case
    hold(got, want, "lds path")
    identical(run(engine, v, mask, 1025, lds_limit=16), got)


def test_two_calls_give_the_same_bytes(engine, mid_case):
    v, mask, _, got = mid_case
    identical(run(engine, v, mask, 1025), got)


def test_a_channel_alone_gives_the_bytes_it_has_among_three(engine, mid_case):
    v, mask, _, got = mid_case
    for c in range(3):
        alone = run(engine, np.ascontiguousarray(v[c:c + 1]), mask, 1025)
        for k in INT_KEYS + BIT_KEYS + VALUE_KEYS:
            assert alone[k][0].tobytes() == got[k][c].tobytes(), (c, k)


def test_poison_behind_m_changes_nothing(engine, mid_case):
    v, mask, _, got = mid_case
    w = v.copy()
    w[:, :, 1025:] = np.nan
    w[:, :, 1025::2] = -np.inf
    identical(run(engine, w, mask, 1025), got)
    identical(run(engine, np.ascontiguousarray(v[:, :, :1025]), mask), got)


def test_end_to_end_on_captured_flights(engine):
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    cap = mc.trajectory_corridor(dict(H.EXAMPLE_IC), 256, stride=25, seed=5, planar=True, nodes=32)
    d = mc.trajectory_depth(cap)
    values, why = cap["values"].cpu().numpy(), cap["reasons"].cpu().numpy()
    want = R.reference(values, why)
    assert d["channels"] == list(cap["channels"]) and np.array_equal(d["time"], cap["time"]) and d["n_masked"] == want["n_masked"]
    for c, name in enumerate(d["channels"]):
        ch = d[name]
        assert same_bits(ch["depth"], want["depth"][c]) and same_bits(ch["mei"], want["mei"][c]), name
        j = ch["median"]
        assert j == want["median"][c] >= 0 and why[j] == 0, "the median flight passes the outlier filter"
        assert same_bits(ch["median_curve"], values[c, :, j])
        assert np.array_equal(ch["central"]["lo"], want["central_lo"][c], equal_nan=True)
        assert np.array_equal(ch["central"]["hi"], want["central_hi"][c], equal_nan=True)
        assert np.array_equal(ch["whisker"]["lo"], want["whisker_lo"][c], equal_nan=True)
        assert same_bits(ch["fence"]["hi"][~np.isnan(want["fence_hi"][c])], want["fence_hi"][c][~np.isnan(want["fence_hi"][c])])
        assert [o["column"] for o in ch["magnitude_outliers"]] == list(np.flatnonzero((want["nodes"][c] > 0) & (want["n_out"][c] > 0)))
        there = np.isfinite(values[c, :, j])
        assert there.any() and np.all((ch["central"]["lo"][there] <= values[c, there, j]) & (values[c, there, j] <= ch["central"]["hi"][there]))
        if ch["shape_outliers"] is not None:
            n = int(want["count"][c][want["count"][c] >= 2][0])
            _, flags = analysis.outliergram(np.where(want["nodes"][c] > 0, want["depth"][c], np.nan), want["mei"][c], n)
            assert ch["shape_outliers"] == list(np.flatnonzero(flags))
