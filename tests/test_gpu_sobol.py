"""erpl_mc_sobol on the device against the NumPy estimators of sobol_ref with the tests' own Philox (philox_ref) on host
copies of the same tensors.

Per replicate, from `replicates_out`: f0, V, S1 and ST of the drawn design rows within the rounding bounds sobol_ref
derives from the drawn data (recursive summation in any order, against a long double evaluation); the bounds are not
tuned to what the device returns, the worst share of a bound is printed.  Per statistic: the counts exact, rep_mean / se /
lo / hi / finite against NumPy on the returned replicates at 1e-12 relative (the bar of test_gpu_bootstrap.py), the
estimates within the same bounds on the population itself."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, models

import helpers as H
import philox_ref
import sobol_ref
from test_gpu_bootstrap import bits, close, interpolate

pytestmark = pytest.mark.gpu

ROW_A, ROW_B, EXTRA = _abi.SUM_FIRST_APOGEE_ALT, _abi.SUM_RAIL_EXIT_SPEED, _abi.SOBOL_ROW_EXTRA
ROWS = [ROW_A, EXTRA, ROW_B]
# (population m of ROW_A and `extra`, factors k, replicates B): below one wave, below and above one workgroup, an odd m (the
# last Philox call half used), k = 1, one chunk of factors exactly (8), the most (32: four chunks), m above one grid row
CASES = [(1, 1, 3), (2, 2, 64), (63, 3, 1), (64, 32, 3), (65, 5, 64), (255, 32, 64), (256, 1, 3), (257, 8, 64), (4099, 32, 16),
         (70001, 3, 8)]


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


def dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def make_inputs(m, k, seed):
    """A [16, ld] summary, an extra row and a mask of a design of n_base = m + 7 rows, ld = (k + 2) n_base + 5.  Three
    design rows are masked; four carry a NaN or an infinity in ROW_A and in `extra`, each in another block (A, B, the first
    and the last AB block): both have m members.  ROW_B is not finite in three of those and in one masked design row: its
    population has m + 1 members.  The outputs share a factor structure (an additive part per factor and a product of the
    first two), so that the indices are of order one."""
    rng = np.random.default_rng(seed)
    n = m + 7
    ld = (k + 2) * n + 5
    summ = rng.normal(size=(_abi.SUMMARY_DIM, ld))
    extra = rng.normal(size=ld)
    A, B = rng.normal(size=(k, n)), rng.normal(size=(k, n))
    w = rng.uniform(0.5, 2.0, size=(3, k))

    def model(X, j):
        return 100.0 * (j + 1) + (w[j][:, None] * X).sum(axis=0) + X[0] * X[k - 1] + 0.1 * X[0] ** 3

    for b in range(k + 2):
        X = A if b == 0 else B if b == 1 else np.vstack([A[:b - 2], B[b - 2:b - 1], A[b - 1:]])
        cols = slice(b * n, (b + 1) * n)
        summ[ROW_A, cols], summ[ROW_B, cols], extra[cols] = model(X, 0), model(X, 1), model(X, 2)
    where = rng.permutation(n)[:7]
    mask = np.zeros(n, dtype=np.uint8)
    mask[where[:3]] = [1, 4, 32]
    blocks = (0, 1, 2, k + 1)
    bad = (np.nan, np.inf, -np.inf, np.nan)
    for j in range(4):
        summ[ROW_A, blocks[j] * n + where[3 + j]] = bad[j]
        extra[blocks[(j + 1) % 4] * n + where[3 + j]] = bad[j]
        if j < 3:
            summ[ROW_B, blocks[(j + 2) % 4] * n + where[3 + j]] = bad[j]
    summ[ROW_B, (k + 1) * n + where[0]] = np.nan     # masked as well: counted as masked
    return summ, extra, mask, n


def population(summ, extra, mask, n, k, row):
    """Y [k + 2, m] of the population of `row`, and (n_masked, n_non_finite)."""
    x = extra if row == EXTRA else summ[row]
    Y = x[:(k + 2) * n].reshape(k + 2, n)
    masked = np.zeros(n, dtype=bool) if mask is None else mask != 0
    fin = np.isfinite(Y).all(axis=0)
    return Y[:, ~masked & fin], int(masked.sum()), int((~masked & ~fin).sum())


def stat_of(out, key, j, k):
    """The (2 + 2 k) values `key` of row j in the order of the replicate matrix."""
    return np.concatenate([[out["mean"][key][j], out["variance"][key][j]], out["first"][key][j], out["total"][key][j]])


def check_summary(out, rep, j, k, level):
    ns, B = 2 + 2 * k, rep.shape[1]
    tail = (1.0 - level) / 2
    got = {key: stat_of(out, key, j, k) for key in ("rep_mean", "se", "lo", "hi", "finite")}
    for s in range(ns):
        theta = rep[j * ns + s]
        theta = theta[np.isfinite(theta)]
        assert got["finite"][s] == len(theta)
        if len(theta) == 0:
            assert all(np.isnan(got[key][s]) for key in ("rep_mean", "se", "lo", "hi"))
            continue
        if theta.min() == theta.max():
            assert got["se"][s] == 0.0 and got["rep_mean"][s] == theta[0]
        else:
            close(got["rep_mean"][s], np.mean(theta))
            close(got["se"][s], np.std(theta, ddof=1))
        srt = np.sort(theta)
        close(got["lo"][s], interpolate(srt, tail))
        close(got["hi"][s], interpolate(srt, 1.0 - tail))


@pytest.mark.parametrize("m,k,B", CASES, ids=[f"m{m}-k{k}-B{B}" for m, k, B in CASES])
def test_replicates_estimates_and_their_summary_against_numpy(engine, m, k, B):
    summ, extra, mask, n = make_inputs(m, k, 3000 + m)
    seed = 91 + m
    out = engine.sobol(dev(engine, summ), n, k, mask=dev(engine, mask), rows=ROWS, extra=dev(engine, extra), replicates=B,
                       level=0.9, seed=seed, want_replicates=True)
    ns = 2 + 2 * k
    rep = out["replicate_values"].cpu().numpy()
    assert rep.shape == (3 * ns, B) and out["rows"] == ROWS and out["replicates"] == B and out["n_base"] == n
    worst = 0.0
    for j, row in enumerate(ROWS):
        Y, n_masked, n_non_finite = population(summ, extra, mask, n, k, row)
        mj = Y.shape[1]
        assert mj == (m + 1 if row == ROW_B else m) and n_masked == 3 and n_non_finite == (3 if row == ROW_B else 4)
        assert (out["count"][j], out["n_masked"][j], out["n_non_finite"][j]) == (mj, n_masked, n_non_finite)
        assert out["constant"][j] == 0
        est = stat_of(out, "estimate", j, k)
        if np.ptp(Y[:2]) == 0:
            assert np.isfinite(est[0])
        else:
            worst = max(worst, sobol_ref.check((est[0], est[1], est[2:2 + k], est[2 + k:]), Y, ("estimate", row)))
        for b in range(B):
            idx = philox_ref.indices(seed, b, mj)
            assert idx.min() >= 0 and idx.max() < mj
            got = rep[j * ns:(j + 1) * ns, b]
            Yb = Y[:, idx]
            if np.ptp(Yb[:2]) == 0:      # one design row drawn throughout, A == B in it: nothing to share out
                assert got[1] == 0.0 and np.isnan(got[2:]).all()
                continue
            worst = max(worst, sobol_ref.check((got[0], got[1], got[2:2 + k], got[2 + k:]), Yb, ("replicate", row, b)))
        check_summary(out, rep, j, k, 0.9)
    print(f"m {m} k {k} B {B}: worst error {worst:.3g} of its bound")


def exact_design(n, k, seed):
    """Y = a function of factor 0 alone: block AB_0 is bitwise B, every other AB block bitwise A.  B's values are A's in
    another order: then sum yB = sum yA and sum yB^2 = sum yA^2, and ST_0 - S1_0 = (sum yA^2 - sum yB^2) / (2 m V) +
    f0 (sum yB - sum yA) / (m V) is zero in exact arithmetic (for two independent samples it is sampling noise)."""
    rng = np.random.default_rng(seed)
    ya = rng.lognormal(3.0, 0.5, n)
    yb = ya[rng.permutation(n)]
    summ = np.zeros((_abi.SUMMARY_DIM, (k + 2) * n))
    summ[ROW_A] = np.concatenate([ya, yb, yb] + [ya] * (k - 1))
    return summ


def test_a_frozen_factor_is_exactly_zero_and_a_lone_factor_is_everything(engine):
    n, k, B = 1031, 9, 32     # two chunks of factors
    summ = exact_design(n, k, 11)
    out = engine.sobol(dev(engine, summ), n, k, rows=[ROW_A], replicates=B, seed=5, want_replicates=True)
    rep = out["replicate_values"].cpu().numpy()
    assert out["count"][0] == n and out["constant"][0] == 0
    # AB_i bitwise A: S1_i = +-0 and ST_i = 0 exactly, in the estimate and in every replicate
    assert np.all(out["first"]["estimate"][0, 1:] == 0.0) and np.all(bits(out["total"]["estimate"][0, 1:]) == 0)
    assert np.all(rep[2 + 1:2 + k] == 0.0) and np.all(bits(rep[2 + k + 1:]) == 0)
    for key in ("rep_mean", "se", "lo", "hi"):
        assert np.all(out["first"][key][0, 1:] == 0.0) and np.all(out["total"][key][0, 1:] == 0.0)
    assert np.all(out["total"]["finite"][0] == B)
    # AB_0 bitwise B, Y a function of factor 0 alone: ST_0 = S1_0 + O(rounding) - each within its bound of the long double
    # value, which is the same for both
    Y = summ[ROW_A].reshape(k + 2, n)
    (_, _, S1, ST), (e0, bV, bS1, bST), solid = sobol_ref.bounds(Y)
    s1, st = out["first"]["estimate"][0, 0], out["total"]["estimate"][0, 0]
    assert solid and abs(ST[0] - S1[0]) <= bS1[0] + bST[0]
    assert abs(s1 - S1[0]) <= bS1[0] and abs(st - ST[0]) <= bST[0] and abs(st - s1) <= 2 * (bS1[0] + bST[0])
    print(f"lone factor: S1 {s1!r}, ST {st!r}, apart {abs(st - s1):.3g}, bound {2 * (bS1[0] + bST[0]):.3g}")
    # near 1: 1 - cov(yA, yB) / V, and a random order leaves a covariance of order V / sqrt(n); five of those
    assert abs(st - 1.0) <= 5.0 / np.sqrt(n)
    assert 0.0 < out["total"]["se"][0, 0] < 0.1


def test_a_constant_row_and_an_empty_population(engine):
    n, k = 300, 2
    summ = np.random.default_rng(3).normal(size=(_abi.SUMMARY_DIM, 4 * n))
    summ[ROW_A, :2 * n] = 0.1            # blocks A and B constant (0.1: sum / count need not be 0.1), the AB blocks not
    summ[ROW_B] = np.nan                 # nothing finite
    out = engine.sobol(dev(engine, summ), n, k, rows=[ROW_A, ROW_B, _abi.SUM_RANGE], replicates=16, want_replicates=True)
    rep = out["replicate_values"].cpu().numpy().reshape(3, 2 + 2 * k, 16)
    assert list(out["constant"]) == [1, 0, 0] and list(out["count"]) == [n, 0, n] and list(out["n_non_finite"]) == [0, n, 0]
    assert abs(out["mean"]["estimate"][0] - 0.1) <= 2 * n * 2.0 ** -53 and out["variance"]["estimate"][0] == 0.0
    assert np.isnan(out["first"]["estimate"][0]).all() and np.isnan(out["total"]["estimate"][0]).all()
    # the empty population: every double NaN, every `finite` 0, every replicate NaN
    for key in ("estimate", "rep_mean", "se", "lo", "hi"):
        assert np.isnan(out["mean"][key][1]) and np.isnan(out["variance"][key][1])
        assert np.isnan(out["first"][key][1]).all() and np.isnan(out["total"][key][1]).all()
    assert out["mean"]["finite"][1] == 0 and not out["first"]["finite"][1].any() and np.isnan(rep[1]).all()
    # the row beside them is alive
    assert out["variance"]["estimate"][2] > 0 and np.isfinite(rep[2]).all() and np.all(out["total"]["finite"][2] == 16)
    # estimates only
    only = engine.sobol(dev(engine, summ), n, k, rows=[_abi.SUM_RANGE], replicates=0)
    assert only["replicates"] == 0 and bits(only["total"]["estimate"][0]).tolist() == bits(out["total"]["estimate"][2]).tolist()
    assert np.isnan(only["total"]["se"]).all() and not only["total"]["finite"].any()
    # a mask that leaves nothing
    none = engine.sobol(dev(engine, summ), n, k, mask=dev(engine, np.full(n, 2, dtype=np.uint8)), rows=[_abi.SUM_RANGE],
                        replicates=4)
    assert (none["count"][0], none["n_masked"][0], none["n_non_finite"][0]) == (0, n, 0) and np.isnan(none["mean"]["estimate"][0])


def frozen(out):
    rest = {key: v for key, v in out.items() if key != "replicate_values"}
    flat = []
    for key in sorted(rest):
        v = rest[key]
        if isinstance(v, dict):
            flat += [(key, sub, bits(v[sub]).tolist() if v[sub].dtype == np.float64 else v[sub].tolist()) for sub in sorted(v)]
        else:
            flat.append((key, v.tolist() if isinstance(v, np.ndarray) else v))
    rep = out.get("replicate_values")
    return flat, None if rep is None else bits(rep.cpu().numpy())


def test_repeatable_whatever_the_workspace_the_stream_and_the_number_of_replicates(engine):
    summ, extra, mask, n = make_inputs(4099, 5, 17)
    args = (dev(engine, summ), n, 5)
    kw = dict(mask=dev(engine, mask), rows=ROWS, extra=dev(engine, extra), seed=31, want_replicates=True)
    a, rep_a = frozen(engine.sobol(*args, replicates=64, **kw))
    b, rep_b = frozen(engine.sobol(*args, replicates=64, **kw))
    assert a == b and np.array_equal(rep_a, rep_b)
    # a call at a larger size regrows the workspace
    big, _, _, nb = make_inputs(20011, 12, 18)
    engine.sobol(dev(engine, big), nb, 12, rows=[ROW_A], replicates=8)
    c, rep_c = frozen(engine.sobol(*args, replicates=64, **kw))
    assert c == a and np.array_equal(rep_c, rep_a)
    side = torch.cuda.Stream(engine.device)
    side.wait_stream(torch.cuda.current_stream(engine.device))
    with torch.cuda.stream(side):
        d, rep_d = frozen(engine.sobol(*args, replicates=64, **kw))
    side.synchronize()
    assert d == a and np.array_equal(rep_d, rep_a)
    # replicate b does not depend on B; the estimates do not either
    e, rep_e = frozen(engine.sobol(*args, replicates=3, **kw))
    assert np.array_equal(rep_e, rep_a.reshape(-1, 64)[:, :3].reshape(rep_e.shape))
    est = lambda f: [x for x in f if x[0] in ("mean", "variance", "first", "total") and x[1] == "estimate"]
    assert est(e) == est(a)
    # replicates_out given or not: the same result struct
    kw.pop("want_replicates")
    f, none = frozen(engine.sobol(*args, replicates=64, **kw))
    assert none is None and f == a
    # another seed is another bootstrap
    _, rep_g = frozen(engine.sobol(*args, replicates=64, **dict(kw, seed=32, want_replicates=True)))
    assert not np.array_equal(rep_g[0], rep_a[0])


def test_ishigami_on_the_device(engine):
    """The design of tests/test_sobol_abi.py: the device's estimates equal the NumPy yardstick to its rounding bound, and
    the yardstick recovers the known indices there - so the device does."""
    Y = sobol_ref.ishigami_design()
    n = Y.shape[1]
    summ = np.zeros((_abi.SUMMARY_DIM, 5 * n))
    summ[ROW_A] = Y.reshape(-1)
    out = engine.sobol(dev(engine, summ), n, 3, rows=[ROW_A], replicates=200, seed=2024)
    s1, st = out["first"]["estimate"][0], out["total"]["estimate"][0]
    worst = sobol_ref.check((out["mean"]["estimate"][0], out["variance"]["estimate"][0], s1, st), Y, "ishigami")
    err = np.abs(np.concatenate([s1 - sobol_ref.ISHIGAMI_S1, st - sobol_ref.ISHIGAMI_ST]))
    print(f"Ishigami on the device: S1 {s1}, ST {st}, largest error {err.max():.4f}, {worst:.3g} of the rounding bound")
    assert np.all(err <= 0.03)
    # the intervals are of the size the error is: every truth within five bootstrap standard errors
    se = np.concatenate([out["first"]["se"][0], out["total"]["se"][0]])
    assert np.all(se > 0) and np.all(se < 0.03) and np.all(err <= 5 * se)


# ------------------------------------------------------------------ the design and the Python layer on real flights
def i64(t):
    """The 64 bits of every double of a device tensor (NaN payloads included)."""
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(
        torch.equal(i64(a.double()), i64(b.double())) if a.dtype != torch.float64 else torch.equal(i64(a), i64(b)))


def same_batch(a, b):
    return all(same_bits(getattr(a, f), getattr(b, f)) for f in ("ic", "rocket", "motor", "alt_grid", "wind", "factors"))


UNC = {"initial_position": [1.0, 2.0, 3.0]}     # a position sigma: otherwise those factor rows are constant


def disperse(engine, n, **kw):
    from erpl_monte_carlo_sim_amd import sampling
    return sampling.synthetic_dispersions(n, models.Rocket(), models.LiquidMotor(), models.WindModel(), dict(H.EXAMPLE_IC),
                                          engine.device, precision=_abi.PREC_F64_FAST, uncertainty=UNC, n_wind_knots=12,
                                          engine=engine, **kw)


def test_the_default_law_is_untouched_and_the_draws_are_the_same_arithmetic(engine):
    """draws=None: two calls agree to the bit and the kept factors are the documented formulae on the generator's z; the
    primitives of the joint law fed through `draws` (z[0:14], z[0:3], z[0:3 K], the uniforms) give the same batch to the
    bit - the independent path is the same arithmetic on other rows."""
    n, K = 300, 12
    a, b = disperse(engine, n, seed=77), disperse(engine, n, seed=77)
    assert same_batch(a, b) and not same_batch(a, disperse(engine, n, seed=78))
    gen = torch.Generator(device=engine.device)
    gen.manual_seed(77)
    z = torch.randn((max(3 * K, 14), n), generator=gen, dtype=torch.float64, device=engine.device)
    uni = torch.rand((2, n), generator=gen, dtype=torch.float64, device=engine.device)
    motor = models.LiquidMotor()
    f = dict(zip(a.factor_names, a.factors))
    col = lambda v: torch.tensor(v, dtype=torch.float64, device=engine.device)
    for c, name in enumerate(("position_x", "position_y", "position_z")):
        assert same_bits(f[name], col(H.EXAMPLE_IC["position"][c]) + col(UNC["initial_position"][c]) * z[c])
    assert same_bits(f["velocity_z"], col(H.EXAMPLE_IC["velocity"][2]) + col(0.1) * z[5])
    assert same_bits(f["mass_multiplier"], 1.0 + 0.02 * z[12])
    assert same_bits(f["motor_thrust_multiplier"], 1.0 + motor.thrust_uncertainty * z[0])
    assert same_bits(f["motor_mass_flow_multiplier"],
                     motor.mass_flow_rate * (1.0 + motor.mass_flow_uncertainty * z[1]) / motor.mass_flow_rate)
    assert same_bits(f["wind_speed"], 0.0 + (5.0 - 0.0) * uni[0])
    joint = torch.cat([z[0:14], z[0:3], z[0:3 * K], uni]).contiguous()
    assert same_batch(disperse(engine, n, draws=joint), a)
    with pytest.raises(ValueError, match="draws"):
        disperse(engine, n, draws=joint[:-1].contiguous())


def test_pick_freeze_blocks_freeze_everything_but_one_group(engine):
    from erpl_monte_carlo_sim_amd import sampling
    n, K = 200, 12
    groups = sampling.primitive_groups(K, liquid=True)
    assert list(groups) == ["position", "velocity", "attitude", "angular_velocity", "mass", "dead_draw", "motor_thrust",
                            "motor_mass_flow", "wind_speed", "wind_direction", "turbulence"]
    assert "motor_mass_flow" not in sampling.primitive_groups(K, liquid=False)
    rows = sorted(r for g in groups.values() for r in g)
    assert len(rows) == len(set(rows)) and set(rows) == set(range(17 + 3 * K + 2)) - {16}
    A, B = sampling.primitive_draws(n, K, engine.device, 5), sampling.primitive_draws(n, K, engine.device, 6)
    assert A.shape == (sampling.primitive_rows(K), n) and bool((A[-2:] >= 0).all() and (A[-2:] < 1).all())
    assert same_bits(A, sampling.primitive_draws(n, K, engine.device, 5)) and not same_bits(A, B)
    # the factor rows (sampling.FACTOR_NAMES) a group moves; the mean wind mixes speed and direction
    moved = {"position": [0, 1, 2], "velocity": [3, 4, 5], "attitude": [6, 7, 8], "angular_velocity": [9, 10, 11],
             "mass": [12], "dead_draw": [], "motor_thrust": [13], "motor_mass_flow": [14], "wind_speed": [15],
             "wind_direction": [16], "turbulence": []}
    mixed = {"wind_speed": [17, 18], "wind_direction": [17, 18]}
    blocks = sampling.pick_freeze_blocks(A, B, groups)
    fa, fb = disperse(engine, n, draws=next(blocks)), disperse(engine, n, draws=next(blocks))
    for name, P in zip(groups, blocks):
        db = disperse(engine, n, draws=P)
        inside = moved[name]
        outside = [r for r in range(19) if r not in inside and r not in mixed.get(name, [])]
        assert same_bits(db.factors[inside], fb.factors[inside]), name
        assert same_bits(db.factors[outside], fa.factors[outside]), name
        for r in inside:
            assert not same_bits(db.factors[r], fa.factors[r]), (name, r)
        windy = name in ("wind_speed", "wind_direction", "turbulence")
        assert same_bits(db.wind, fa.wind) != windy, name
        if name == "dead_draw":
            assert same_batch(db, fa)
    # groups must be disjoint, at most 32, inside the tensor
    with pytest.raises(ValueError, match="disjoint"):
        list(sampling.pick_freeze_blocks(A, B, {"a": [0, 1], "b": [1]}))
    with pytest.raises(ValueError, match="groups"):
        list(sampling.pick_freeze_blocks(A, B, {f"g{i}": [i] for i in range(33)}))
    with pytest.raises(ValueError, match="outside"):
        list(sampling.pick_freeze_blocks(A, B, {"a": [A.shape[0]]}))


def test_sobol_indices_of_real_flights_end_to_end(engine):
    from erpl_monte_carlo_sim_amd import sampling
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    an = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    names = ["mass", "motor_thrust", "dead_draw"]
    out = an.sobol_indices(dict(H.EXAMPLE_IC), n_base=256, groups=names, planar=True, replicates=100, seed=1234)
    assert out["group_names"] == names and out["n_base"] == 256 and out["summary"].shape == (16, 5 * 256)
    assert out["row_names"] == ["first_apogee_altitude", "first_apogee_time", "rail_exit_speed"]
    assert out["groups"] == {"mass": [12], "motor_thrust": [14], "dead_draw": [13]} and out["mask"] is None
    assert list(out["count"]) == [256, 256, 256] and not out["constant"].any()
    st, s1 = out["total"]["estimate"], out["first"]["estimate"]
    print(f"S1 {s1.tolist()}\nST {st.tolist()}\ninteraction {out['interaction'].tolist()}")
    # the reference draws a thrust multiplier it never uses: it reaches no output, to the bit
    assert np.all(bits(st[:, 2]) == 0) and np.all(s1[:, 2] == 0.0)
    assert np.all(out["total"]["hi"][:, 2] == 0.0) and np.all(out["total"]["se"][:, 2] == 0.0)
    assert np.all(st[:, :2] > 0.0) and np.all(out["total"]["lo"][:, :2] > 0.0)
    for j in range(3):
        assert out["ranking"][j][2] == "dead_draw" and set(out["ranking"][j][:2]) == {"mass", "motor_thrust"}
    np.testing.assert_array_equal(out["sum_first"], s1.sum(axis=1))
    np.testing.assert_array_equal(out["interaction"], 1.0 - out["sum_first"])
    # block A is a plain run of the same primitives
    eng = shared_engine(an.device)
    A = sampling.primitive_draws(256, 100, eng.device, 1234)
    db = sampling.synthetic_dispersions(256, an.rocket, an.motor, an.wind_model, dict(H.EXAMPLE_IC), eng.device,
                                        precision=_abi.PREC_F64_FAST, uncertainty=an.uncertainty_params, planar=True,
                                        engine=eng, draws=A)
    summ, status = eng.run(db)
    torch.cuda.synchronize(eng.device)
    assert same_bits(out["summary"][:, :256], summ) and torch.equal(out["status"][:256], status)
    # with the outlier filter the mask is the OR of the reasons over the blocks; nothing here is an outlier of every block
    filt = an.sobol_indices(dict(H.EXAMPLE_IC), n_base=256, groups=names, planar=True, replicates=0, filter_outliers=True)
    assert filt["mask"].shape == (256,) and filt["mask"].dtype == torch.uint8
    kept = int((filt["mask"] == 0).sum())
    assert list(filt["count"]) == [kept] * 3 and list(filt["n_masked"]) == [256 - kept] * 3
    with pytest.raises(ValueError, match="unknown group"):
        an.sobol_indices(dict(H.EXAMPLE_IC), n_base=8, groups=["thrust"])
