"""erpl_mc_subset_* on the device: every step against its host twin (the same header code, itself held to the restatement
subset_ref by test_subset_abi.py) and against the restatement - never device against itself alone; the whole run on the linear
limit state against the exact probabilities and the host run; and MonteCarloAnalyzer.rare_event over flights."""
import math

import numpy as np
import pytest
import torch
from scipy import special

from erpl_monte_carlo_sim_amd import _abi, analysis, models, sampling

import helpers as H
import subset_cases as SC
import subset_ref as R

linear_draws0 = SC.linear_draws0

pytestmark = pytest.mark.gpu


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 7. the steps
def device_propose(engine, step, level, cur, first_chain=0, rho=SC.PROPOSE_RHO, w=SC.PROPOSE_W):
    """cur: a NumPy [5, count] block; on the device it sits in a wider matrix (ld > count), and so does the output."""
    count = cur.shape[1]
    wide = torch.full((5, count + 7), 55.0, dtype=torch.float64, device="cuda")
    wide[:, :count] = dev(cur)
    out = torch.full((5, count + 3), -7.0, dtype=torch.float64, device="cuda")
    spec = analysis.subset_spec(seed=SC.PROPOSE_SEED, level=level, step=step)
    engine.subset_propose(spec, SC.PROPOSE_KINDS, rho, wide[:, :count], first_chain, out[:, :count], w=w)
    got = host(out)
    assert np.all(got[:, count:] == -7.0)
    return got[:, :count]


@pytest.mark.parametrize("chains", (SC.PROPOSE_CHAINS, 65, 257))
@pytest.mark.parametrize("step,level", SC.PROPOSE_POINTS)
def test_device_proposals(engine, step, level, chains):
    cur = np.ascontiguousarray(SC.propose_current(chains, chains + 7)[:, :chains])
    got = device_propose(engine, step, level, cur)
    SC.check_proposal(got, cur, step, level)                       # the restatement: uniform rows to the bit
    spec = analysis.subset_spec(seed=SC.PROPOSE_SEED, level=level, step=step)
    twin = analysis.subset_propose_host(spec, SC.PROPOSE_KINDS, SC.PROPOSE_RHO, cur, w=SC.PROPOSE_W)
    assert np.array_equal(got[3:].view(np.uint64), twin[3:].view(np.uint64))
    s = np.sqrt(1.0 - SC.PROPOSE_RHO ** 2)
    _, xi = R.propose(cur, SC.PROPOSE_KINDS, SC.PROPOSE_RHO, s, SC.PROPOSE_W, SC.PROPOSE_SEED, level, step)
    for r in range(3):                                             # host and device: within twice the header's bound
        assert np.all(np.abs(got[r] - twin[r]) <= 2 * R.normal_bar(cur[r], xi[r], SC.PROPOSE_RHO[r], s[r])), r
    if chains == SC.PROPOSE_CHAINS:
        first, count = SC.WINDOW
        win = device_propose(engine, step, level, cur[:, first:first + count], first_chain=first)
        assert np.array_equal(win.view(np.uint64), got[:, first:first + count].view(np.uint64))


def test_device_proposals_with_rho_0_and_1(engine):
    cur = np.ascontiguousarray(SC.propose_current()[:, :SC.PROPOSE_CHAINS])
    fresh = device_propose(engine, 1, 0, cur, rho=np.zeros(5))
    copy = device_propose(engine, 1, 0, cur, rho=np.ones(5), w=np.zeros(5))
    xi = special.ndtri(R.uniforms(SC.PROPOSE_SEED, 0, 1, 3, 0, SC.PROPOSE_CHAINS))
    assert np.all(np.abs(fresh[:3] - xi) <= 8e-15 * np.maximum(1.0, np.abs(xi)))
    assert np.array_equal(copy[:3], cur[:3]) and np.array_equal(copy[3:, 8:], cur[3:, 8:])


@pytest.mark.parametrize("name,g,n_seeds", SC.seed_cases(), ids=[c[0] for c in SC.seed_cases()])
def test_device_seed_selection(engine, name, g, n_seeds):
    """All four gather slots: a 5-row matrix of doubles, a 16-row summary, an int32 status row and g itself."""
    n = g.size
    rng = np.random.default_rng(n)
    prim, summ, status = rng.normal(size=(5, n)), rng.normal(size=(16, n)), rng.integers(0, 1 << 12, n).astype(np.int32)
    d_out = [torch.full((5, n_seeds + 2), -1.0, dtype=torch.float64, device="cuda"), torch.full((16, n_seeds), -1.0, dtype=torch.float64, device="cuda"),
             torch.full((n_seeds + 1,), -1, dtype=torch.int32, device="cuda"), torch.full((n_seeds,), -1.0, dtype=torch.float64, device="cuda")]
    dg = dev(g)
    idx, sel, thr, alive = engine.subset_seeds(dg, n_seeds, [(dev(prim), d_out[0][:, :n_seeds]), (dev(summ), d_out[1]),
                                                             (dev(status), d_out[2][:n_seeds]), (dg, d_out[3])])
    idx, sel, thr, alive = host(idx), host(sel), float(host(thr)), int(host(alive))
    SC.check_seeds(g, n_seeds, idx, sel, thr, alive)                # the restatement
    h_idx, h_sel, h_thr, h_alive = analysis.subset_seeds_host(g, n_seeds)
    assert np.array_equal(idx, h_idx) and np.array_equal(sel, h_sel) and alive == h_alive     # the host twin
    got = [host(t) for t in d_out]
    assert np.array_equal(got[0][:, :n_seeds], prim[:, idx]) and np.all(got[0][:, n_seeds:] == -1.0)
    assert np.array_equal(got[1], summ[:, idx]) and np.array_equal(got[2][:n_seeds], status[idx]) and got[2][n_seeds] == -1
    assert np.array_equal(got[3].view(np.uint64), g[idx].view(np.uint64))
    thr_t = torch.tensor(thr, dtype=torch.float64, device="cuda")
    _, ind, _, count = engine.subset_seeds(dg, 0, threshold=thr_t)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(host(ind), (g >= thr).astype(np.uint8)) and int(host(count)) == int((g >= thr).sum())


def test_device_seed_selection_reports_a_died_out_level(engine):
    g = np.array([1.0, -np.inf, np.nan, 2.0, -np.inf] * 30)
    _, _, _, alive = engine.subset_seeds(dev(g), 61)
    assert int(host(alive)) == 60                                    # the caller's comparison: 60 < 61
    dead = lambda d: torch.where(torch.arange(d.shape[1], device="cuda") < 10, d[0], torch.full_like(d[0], -math.inf))
    x = dev(linear_draws0(3)[:, :256])
    with pytest.raises(ValueError, match="fewer than chains"):
        analysis.subset_simulation(dead, x, SC.LINEAR_KINDS, chains=64, steps=4, engine=engine)


@pytest.mark.parametrize("name,sel,chains,steps", SC.chain_cases(), ids=[c[0] for c in SC.chain_cases()])
def test_device_chain_statistics(engine, name, sel, chains, steps):
    n1, pair = engine.subset_chain_stats(dev(sel), chains, steps)
    w_n1, w_pair = R.chain_stats(sel, chains, steps)
    h_n1, h_pair = analysis.subset_chain_stats_host(sel, chains, steps)
    assert int(host(n1)) == w_n1 == h_n1 and np.array_equal(host(pair), w_pair) and np.array_equal(h_pair, w_pair)


@pytest.mark.parametrize("count", (130, 65, 257))
@pytest.mark.parametrize("mode", ("mixed", "all", "none"))
def test_device_commit(engine, count, mode):
    """All four triples (5 rows of doubles, a 16-row summary, an int32 status row, a byte row) next to g; candidates equal to
    the threshold, just below it, NaN and +inf."""
    rng = np.random.default_rng(count)
    g_cur, g_cand = rng.normal(size=count), rng.normal(size=count)
    thr = 0.25
    if mode == "mixed":
        g_cand[:4] = [thr, np.nextafter(thr, 0.0), np.nan, np.inf]
    g_cand = g_cand if mode == "mixed" else (np.abs(g_cand) + thr if mode == "all" else -np.abs(g_cand))
    shapes = ((5, np.float64), (16, np.float64), (1, np.int32), (1, np.uint8))
    cand = [rng.integers(0, 200, (rows, count)).astype(dt) for rows, dt in shapes]
    pop = [rng.integers(0, 200, (rows, 2 * count + 3)).astype(dt) for rows, dt in shapes]
    g_pop = np.concatenate([g_cur, np.full(count + 3, -9.0)])
    # the host twin, in place
    h_pop, h_g = [p.copy() for p in pop], g_pop.copy()
    squeeze = lambda a: a[0] if a.shape[0] == 1 else a
    acc = analysis.subset_commit_host(thr, g_cand, h_g[:count], h_g[count:2 * count],
                                      [(squeeze(c), squeeze(p[:, :count]), squeeze(p[:, count:2 * count])) for c, p in zip(cand, h_pop)])
    take = g_cand >= thr
    assert acc == int(take.sum()) and acc == {"all": count, "none": 0}.get(mode, acc)
    # the device
    d_pop, d_g, d_cand = [dev(p) for p in pop], dev(g_pop), [dev(c) for c in cand]
    n_acc = torch.full((), 1000, dtype=torch.int64, device="cuda")
    engine.subset_commit(torch.tensor(thr, dtype=torch.float64, device="cuda"), dev(g_cand), d_g[:count], d_g[count:2 * count],
                         [(squeeze(c), squeeze(p[:, :count]), squeeze(p[:, count:2 * count])) for c, p in zip(d_cand, d_pop)], n_acc)
    assert int(host(n_acc)) == 1000 + acc                            # added to
    assert np.array_equal(host(d_g).view(np.uint64), h_g.view(np.uint64))
    for q in range(4):
        assert np.array_equal(host(d_pop[q]), h_pop[q]), q
        assert np.array_equal(h_pop[q][:, count:2 * count], np.where(take, cand[q], pop[q][:, :count])), q      # the rule itself
        assert np.array_equal(h_pop[q][:, 2 * count:], pop[q][:, 2 * count:])


# ------------------------------------------------------------------------------------------------ 8. the limit state
def test_device_limit_state_equals_the_host_twin(engine):
    summ, status = SC.limit_state_inputs()
    wide = torch.full((16, 1025 + 5), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :1025] = dev(summ)
    for name, spec, kw in SC.limit_state_specs():
        kw = dict(kw)
        want = R.limit_state(summ, status, kw.pop("bounds", SC.BOUNDS), **kw)
        twin = analysis.subset_limit_state_host(spec, summ, status)
        got = host(engine.subset_limit_state(spec, wide[:, :1025], dev(status)))
        assert np.array_equal(got.view(np.uint64), twin.view(np.uint64)), name
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    spec = SC.limit_state_specs()[0][1]
    assert np.array_equal(host(engine.subset_limit_state(spec, dev(summ), None)), analysis.subset_limit_state_host(spec, summ, None))


# ------------------------------------------------------------------------------------------------ 9. the whole run
def linear_g_device(x):
    """The host's operation order, element by element: the rows added one by one, then the weight."""
    acc = x[0].clone()
    for r in range(1, 22):
        acc = acc + x[r]
    return acc * SC.LINEAR_WEIGHT


@pytest.mark.parametrize("target,exact,sized_cov,seed", SC.LINEAR_TARGETS)
def test_linear_limit_state_on_the_device(engine, target, exact, sized_cov, seed):
    chains, steps = SC.LINEAR_CHAINS, SC.LINEAR_STEPS
    x0 = linear_draws0(seed)
    out = analysis.subset_simulation(linear_g_device, dev(x0), SC.LINEAR_KINDS, chains=chains, steps=steps, target=target,
                                     rho=SC.LINEAR_RHO, seed=seed, engine=engine)
    ratio = SC.check_linear(out, exact, sized_cov)
    ref = analysis.subset_simulation(SC.linear_g, x0, SC.LINEAR_KINDS, chains=chains, steps=steps, target=target, rho=SC.LINEAR_RHO, seed=seed)
    print(f"target {target}: device P = {out['probability']:.6g}, cov = {out['cov']:.4f}, ratio = {ratio:.3f}; host P = {ref['probability']:.6g}; "
          f"counts {[lv['n1'] for lv in out['levels']]} / {[lv['n1'] for lv in ref['levels']]}")
    assert [lv["n1"] for lv in out["levels"]] == [lv["n1"] for lv in ref["levels"]]
    assert np.allclose(out["thresholds"], ref["thresholds"], rtol=1e-12, atol=0)
    assert out["evaluations"] == ref["evaluations"] and out["samples"] == ref["samples"]
    pop = out["population"]
    assert np.array_equal(host(pop["indicator"]), (host(pop["g"]) >= target).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ 10. flights
RARE = dict(n_per_level=512, p0=0.25, max_levels=2, target=None, planar=True, seed=77)


@pytest.fixture(scope="module")
def rare(analyzer):
    return analyzer.rare_event(dict(H.EXAMPLE_IC), **RARE)


def population_bytes(out):
    pop = out["population"]
    return b"".join(host(pop[k]).tobytes() for k in ("draws", "summary", "status", "g", "indicator")) + repr(out["thresholds"]).encode()


def test_rare_event_level_0_is_the_design_run(analyzer, rare):
    run = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 512, seed=77, planar=True, design="random")
    assert host(rare["level0"]["summary"]).tobytes() == host(run["summary"]).tobytes()
    assert np.array_equal(host(rare["level0"]["status"]), host(run["status"]))


def test_rare_event_population_lies_beyond_its_thresholds(engine, rare):
    thr = rare["thresholds"]
    assert len(thr) == 2 and thr[1] > thr[0] and rare["probability"] == 0.25 ** 2
    pop = rare["population"]
    summ, status, g = pop["summary"], pop["status"], host(pop["g"])
    _, why = engine.analyze(summ.contiguous(), status.contiguous(), reasons=True)
    assert not host(why).any() and np.all(g >= thr[1]) and np.all(host(pop["indicator"]) == 1)
    assert np.array_equal(g, host(summ)[_abi.SUM_RANGE])
    assert rare["evaluations"] == 512 + 2 * 3 * 128 == rare["performance"]["flights"]
    assert set(rare["conditional_inputs"]) == set(sampling.scalar_primitives(100, True))
    assert all(0.0 < lv["acceptance"] <= 1.0 for lv in rare["levels"])


def test_rare_event_population_flies_again_to_the_bit(analyzer, rare):
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    eng = shared_engine(analyzer.device)
    pop = rare["population"]
    db = sampling.synthetic_dispersions(512, analyzer.rocket, analyzer.motor, analyzer.wind_model, dict(H.EXAMPLE_IC), eng.device,
                                        precision=_abi.PRECISIONS["f64_fast"], uncertainty=analyzer.uncertainty_params, planar=True,
                                        engine=eng, draws=pop["draws"].contiguous())
    summ, status = eng.run(db)[:2]
    eng.synchronize()
    assert host(summ).tobytes() == host(pop["summary"]).tobytes() and np.array_equal(host(status), host(pop["status"]))


def test_rare_event_is_repeatable_and_independent_of_the_sub_batches(analyzer, rare, monkeypatch):
    want = population_bytes(rare)
    assert population_bytes(analyzer.rare_event(dict(H.EXAMPLE_IC), **RARE)) == want
    monkeypatch.setattr(analyzer, "DEVICE_CHUNK", 128)
    assert population_bytes(analyzer.rare_event(dict(H.EXAMPLE_IC), **RARE)) == want


def test_rare_event_refusals(analyzer):
    for kw in (dict(p0=0.3), dict(p0=1.0), dict(n_per_level=510, p0=0.25), dict(design="sobol")):
        with pytest.raises(ValueError):
            analyzer.rare_event(dict(H.EXAMPLE_IC), **{**RARE, **kw})


# ------------------------------------------------------------------------------------------------ 11. direct Monte Carlo
def test_rare_event_agrees_with_direct_monte_carlo(analyzer):
    """x* = the 98th percentile of g (the range; -inf for a flight the filter drops, about a fifth of the planar set) over ALL
    8192 flights of another seed, so that 2 % of all flights lie beyond it; P(g >= x*) by subset simulation at
    n_per_level = 1024, p0 = 1/4 against 0.02: |ln(P / 0.02)| <= 4 sqrt(cov^2 + (1 - 0.02) / (0.02 * 8192)).
    Measured: x* = 7861.6 m, P = 0.01353, cov = 0.124, |ln(P / 0.02)| = 0.39, bound 0.59."""
    run = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 8192, seed=4321, planar=True, design="random")
    spec = analysis.subset_spec()
    g = host(shared(analyzer).subset_limit_state(spec, run["summary"].contiguous(), run["status"].contiguous()))
    x_star = float(np.percentile(g, 98.0))
    out = analyzer.rare_event(dict(H.EXAMPLE_IC), n_per_level=1024, p0=0.25, target=x_star, planar=True, seed=99)
    bound = 4.0 * math.sqrt(out["cov"] ** 2 + (1 - 0.02) / (0.02 * 8192))
    ratio = abs(math.log(out["probability"] / 0.02))
    print(f"x* = {x_star:.3f} m: P = {out['probability']:.5f}, cov = {out['cov']:.4f}, |ln(P / 0.02)| = {ratio:.4f}, bound = {bound:.4f}, "
          f"levels = {len(out['levels'])}, evaluations = {out['evaluations']}")
    assert out["reached"] and ratio <= bound


def shared(analyzer):
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    return shared_engine(analyzer.device)
