"""erpl_mc_design on the device against erpl_mc_design_host (the same header code on the host, itself held to design_ref by
test_design_abi.py): probabilities and ranks bit for bit, normal rows against scipy's normal quantile of the host's p; and
the design flown: run_monte_carlo_device(design=...), its replicates and their intervals, sobol_indices(design=...)."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models, sampling

import design_cases as DC
import helpers as H

pytestmark = pytest.mark.gpu

U, N = _abi.DESIGN_UNIFORM, _abi.DESIGN_NORMAL
KINDS = (_abi.DESIGN_RANDOM, _abi.DESIGN_LHS, _abi.DESIGN_LHS_CENTRED)
SENTINEL = -7.25


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def analyzer():
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    return MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)


def device_design(engine, kind, kinds, n, block=0, first=0, count=None, first_row=0, seed=DC.SEED, pad=3):
    """TrajectoryEngine.design into the first `count` columns of a [rows, count + pad] tensor full of sentinels."""
    count = n - first if count is None else count
    out = torch.full((len(kinds), count + pad), SENTINEL, dtype=torch.float64, device=engine.device)
    got = engine.design(kinds, n, seed, kind=kind, block=block, first=first, count=count, first_row=first_row, out=out)
    assert got is out
    engine.synchronize()        # the blocking check that reports a cycle walk given up on the device
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", DC.SHAPES, ids=DC.shape_id)
def test_device_design_equals_the_host_copy(engine, shape):
    rows, n, block, first, count, first_row = shape
    m = block or n
    mixed = [N if r % 2 == 0 else U for r in range(rows)]
    for kind in KINDS:
        host_p = DC.host_design(engine.lib, kind, [U] * rows, n, block, first, count, first_row)
        got_p = device_design(engine, kind, [U] * rows, n, block, first, count, first_row)
        assert np.array_equal(got_p[:, :count], host_p), kind
        assert np.all(got_p[:, count:] == SENTINEL)              # [.., count .. ld - 1] is never written
        again = device_design(engine, kind, [U] * rows, n, block, first, count, first_row)
        assert got_p.tobytes() == again.tobytes()
        got = device_design(engine, kind, mixed, n, block, first, count, first_row, pad=0)
        assert np.array_equal(got[1::2], host_p[1::2])
        DC.assert_normals(got[0::2], host_p[0::2])
        if n <= 70000:      # the window equals those columns of the full call; ranks within the replicates as on the host
            full = device_design(engine, kind, mixed, n, block, 0, n, first_row, pad=0)
            assert np.array_equal(full[:, first:first + count], got)
            if kind == _abi.DESIGN_LHS:
                host_full = DC.host_design(engine.lib, kind, [U] * rows, n, block, 0, n, first_row)
                assert np.array_equal(DC.ranks_in_replicates(full, m), DC.ranks_in_replicates(host_full, m))


def test_count_zero_writes_nothing_and_a_default_tensor_has_the_right_shape(engine):
    out = torch.full((2, 3), SENTINEL, dtype=torch.float64, device=engine.device)
    engine.design([N, U], 12, 1, first=12, count=0, out=out)
    engine.synchronize()
    assert bool((out == SENTINEL).all())
    got = engine.design([N, U, U], 300, 1, first=100)
    assert tuple(got.shape) == (3, 200) and got.dtype == torch.float64 and got.device == engine.device
    d = sampling.design_draws(64, 6, engine.device, 5, engine=engine)
    assert tuple(d.shape) == (sampling.primitive_rows(6), 64)
    z, u = d[:-2].cpu().numpy(), d[-2:].cpu().numpy()
    assert np.all((u > 0) & (u < 1)) and np.array_equal(np.sort(np.floor(u * 64), axis=1), np.tile(np.arange(64.0), (2, 1)))
    # 64 strata: the outermost values lie beyond ndtri(63 / 64) = 2.1539; the mean of such a row has a standard deviation of
    # about 0.006 (the two tail strata, 0.7 wide in z, carry it), an i.i.d. row one of 0.125
    assert np.all(z.max(axis=1) > 2.1538) and np.all(z.min(axis=1) < -2.1538) and np.abs(z.mean(axis=1)).max() < 0.05


def test_lhs_cuts_the_variance_of_a_near_additive_mean_on_the_device(engine):
    """The variance property of test_design_abi.py with 64 seeds, the designs drawn by the kernel."""
    est = {kind: [DC.additive_estimator(engine.design([N] * 20, 256, s, kind=kind).cpu().numpy()) for s in range(64)]
           for kind in ("random", "lhs")}
    engine.synchronize()
    ratio = np.var(est["lhs"]) / np.var(est["random"])
    print(f"variance ratio LHS / RANDOM = {ratio:.5f}")
    assert ratio <= 0.05


def _strata(out, analyzer, block):
    names = out["factor_names"]
    ws = out["factors"][names.index("wind_speed")].cpu().numpy()
    lo, hi = analyzer.uncertainty_params["wind_speed_range"]
    return np.floor((ws - lo) / (hi - lo) * block).astype(np.int64)


@pytest.fixture(scope="module")
def lhs_run(analyzer):
    return analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 512, design="lhs", keep_factors=True)


def test_a_design_run_is_stratified(lhs_run, analyzer):
    assert np.array_equal(np.sort(_strata(lhs_run, analyzer, 512)), np.arange(512))
    assert lhs_run["design"] == {"kind": "lhs", "seed": 1234, "block": 512, "replicates": 1}
    with pytest.raises(ValueError, match="design_replicates"):
        analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 512, design="lhs", design_replicates=5)
    with pytest.raises(ValueError, match="design"):
        analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 512, design="sobol")


def test_a_design_run_does_not_depend_on_the_sub_batches(lhs_run, analyzer, monkeypatch):
    monkeypatch.setattr(analyzer, "DEVICE_CHUNK", 512)
    one = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 512, design="lhs")
    monkeypatch.setattr(analyzer, "DEVICE_CHUNK", 128)
    four = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 512, design="lhs")
    assert four["performance"]["sub_batches"] == 4 and one["performance"]["sub_batches"] == 1
    for other in (one, lhs_run):
        assert four["summary"].cpu().numpy().tobytes() == other["summary"].cpu().numpy().tobytes()
        assert torch.equal(four["status"], other["status"])


def test_replicates_are_stratified_blocks_with_a_valid_interval(analyzer):
    out = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 512, design="lhs", keep_factors=True, design_replicates=4)
    assert out["design"] == {"kind": "lhs", "seed": 1234, "block": 128, "replicates": 4}
    strata = _strata(out, analyzer, 128).reshape(4, 128)
    assert np.array_equal(np.sort(strata, axis=1), np.tile(np.arange(128), (4, 1)))
    assert not np.array_equal(strata[0], strata[1])
    rows = [_abi.SUM_FIRST_APOGEE_ALT, _abi.SUM_RAIL_EXIT_SPEED]
    ri = analysis.replicate_intervals(out["summary"], out["status"], 128, rows=rows)
    assert (ri["replicates"], ri["block"], ri["level"]) == (4, 128, 0.95)
    for r in rows:
        s = ri[analysis.ROW_NAMES[r]]
        means = np.asarray(s["replicate_means"])
        assert means.shape == (4,) and np.all(np.isfinite(means)) and sum(s["replicate_counts"]) > 0
        assert s["mean"] == float(np.mean(means)) and s["lo"] < s["mean"] < s["hi"] and s["se"] > 0
        # Student t, 3 degrees of freedom, 97.5 %: 3.182446
        assert abs((s["hi"] - s["mean"]) - 3.182446305284263 * np.std(means, ddof=1) / 2.0) <= 1e-9 * abs(s["hi"])
    with pytest.raises(ValueError, match="block"):
        analysis.replicate_intervals(out["summary"], out["status"], 100)


def test_sobol_indices_fly_a_design(analyzer, monkeypatch):
    seen = []
    real = sampling.synthetic_dispersions

    def spy(*a, **kw):
        seen.append(kw["draws"])
        return real(*a, **kw)

    monkeypatch.setattr(sampling, "synthetic_dispersions", spy)
    out = analyzer.sobol_indices(dict(H.EXAMPLE_IC), n_base=64, design="lhs", groups=["mass", "wind_speed"], replicates=50)
    assert out["design"]["kind"] == "lhs" and len(seen) == 4 and out["n_base"] == 64
    row = out["groups"]["wind_speed"][0]
    a_block = seen[0][row].cpu().numpy()
    assert np.array_equal(np.sort(np.floor(a_block * 64)), np.arange(64.0))
    b_block = seen[1][row].cpu().numpy()
    assert np.array_equal(np.sort(np.floor(b_block * 64)), np.arange(64.0)) and not np.array_equal(a_block, b_block)
    assert np.array_equal(seen[3][row].cpu().numpy(), b_block)       # AB of wind_speed: that row from B
    assert out["group_names"] == ["mass", "wind_speed"] and np.asarray(out["first"]["estimate"]).shape[1] == 2
