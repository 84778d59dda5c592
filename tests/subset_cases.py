"""What test_subset_abi.py (host) and test_gpu_subset.py (device) share: the shapes, the inputs and the yardsticks of the
five steps of erpl_mc_subset_* against subset_ref."""
import math

import numpy as np

import subset_ref as R
from erpl_monte_carlo_sim_amd import _abi, analysis

# ---- proposals: R = 5 (3 normal, 2 uniform), 130 chains, ld > count
PROPOSE_KINDS = (1, 1, 1, 0, 0)
PROPOSE_CHAINS, PROPOSE_LD = 130, 137
PROPOSE_RHO = np.array([0.8, 0.5, 0.95, 0.0, 0.0])
PROPOSE_W = np.array([0.0, 0.0, 0.0, 0.6, 1.0])
PROPOSE_POINTS = tuple((step, level) for step in (1, 65535) for level in (0, 2 ** 32 - 1))
PROPOSE_SEED = 0x9E3779B97F4A7C15
WINDOW = (37, 29)     # first_chain, count


def propose_current(chains=PROPOSE_CHAINS, ld=PROPOSE_LD):
    """The current states [5, ld], columns chains .. ld - 1 a sentinel: normals, and uniforms that sit at both ends of (0, 1)
    in the first columns so that steps wrap below 0 and above 1."""
    rng = np.random.default_rng(11)
    cur = np.full((5, ld), 123.0)
    cur[:3, :chains] = rng.standard_normal((3, chains))
    cur[3:, :chains] = rng.random((2, chains))
    cur[3:, 0:8] = [[1e-3, 1 - 1e-3, 2.0 ** -60, 1 - 2.0 ** -53, 0.01, 0.99, 5e-324, 0.5]] * 2
    return cur


def check_proposal(got, cur, step, level, first_chain=0, rho=PROPOSE_RHO, w=PROPOSE_W):
    """Uniform rows bit for bit, normal rows within the header's bound of rho x + s ndtri(u)."""
    s = np.sqrt(1.0 - rho * rho)
    want, xi = R.propose(cur, PROPOSE_KINDS, rho, s, w, PROPOSE_SEED, level, step, first_chain)
    for r, kind in enumerate(PROPOSE_KINDS):
        if kind == R.UNIFORM:
            assert np.array_equal(got[r].view(np.uint64), want[r].view(np.uint64)), (r, step, level)
            assert np.all((got[r] > 0.0) & (got[r] < 1.0))
        else:
            err = np.abs(got[r] - want[r])
            assert np.all(err <= R.normal_bar(cur[r], xi[r], rho[r], s[r])), (r, step, level, err.max())
    return want


# ---- seed selection
def seed_cases():
    """(name, g, n_seeds): integer-valued g with ties across the threshold, all equal, -inf / NaN / zeros of both signs,
    n_seeds = 1 and = n, n = 1, 63, 64, 65, 1025."""
    rng = np.random.default_rng(5)
    out = []
    for n in (1, 63, 64, 65, 1025, 4099):
        ties = rng.integers(0, 7, n).astype(np.float64)
        for k in sorted({1, max(1, n // 8), max(1, n // 2), n}):
            out.append((f"ties-{n}-{k}", ties, k))
        out.append((f"equal-{n}", np.full(n, 2.5), max(1, n // 3)))
    mixed = rng.integers(-2, 3, 1025).astype(np.float64)
    mixed[::7] = -np.inf
    mixed[3::11] = np.nan
    mixed[5::13] = -0.0
    mixed[6::13] = 0.0
    alive = int(np.count_nonzero(mixed > -np.inf))
    for k in (1, 100, alive - 1, alive):
        out.append((f"mixed-{k}", mixed, k))
    # the threshold falls between -0.0 and +0.0
    zeros = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0])
    for k in (1, 2, 4, 5, 7, 8):
        out.append((f"zeros-{k}", zeros, k))
    return out


def check_seeds(g, n_seeds, idx, sel, thr, alive):
    w_idx, w_sel, w_thr, w_alive = R.seeds(g, n_seeds)
    assert np.array_equal(idx, w_idx) and np.array_equal(sel, w_sel) and alive == w_alive
    assert np.array([thr]).view(np.uint64)[0] == np.array([w_thr]).view(np.uint64)[0], (thr, w_thr)


# ---- chain statistics
def chain_cases():
    rng = np.random.default_rng(3)
    out = []
    for chains, steps in ((130, 5), (1, 2), (65, 3), (257, 8), (7, 1)):
        n = chains * steps
        one = np.zeros((steps, chains), dtype=np.uint8)
        one[:, chains // 2] = 1
        for name, sel in (("random", (rng.random(n) < 0.4).astype(np.uint8)), ("ones", np.ones(n, dtype=np.uint8)),
                          ("zeros", np.zeros(n, dtype=np.uint8)), ("one-chain", one.reshape(-1)), ("bytes", rng.integers(0, 3, n).astype(np.uint8) * 100)):
            out.append((f"{chains}x{steps}-{name}", sel, chains, steps))
    return out


# ---- the limit state: a 1025-column summary built by hand
BOUNDS = (80000.0, 100.0, 200000.0, 600.0, 1200.0 ** 2 / (2 * 9.81) * 1.2)


def limit_state_inputs(n=1025):
    rng = np.random.default_rng(17)
    summ = rng.normal(0.0, 1.0, (16, n))
    summ[R.APOGEE] = rng.uniform(1000.0, 50000.0, n)
    summ[R.RANGE] = rng.uniform(100.0, 150000.0, n)
    summ[R.FLIGHT_TIME] = rng.uniform(10.0, 500.0, n)
    summ[R.IMPACT_X] = rng.normal(0.0, 3e4, n)
    summ[R.IMPACT_Y] = rng.normal(0.0, 3e4, n)
    status = rng.integers(0, 5, n).astype(np.int32)
    summ[R.APOGEE, 3] = np.nan                 # NON_FINITE
    summ[R.FLIGHT_TIME, 4] = np.inf            # NON_FINITE (and FLIGHT_TIME)
    summ[R.APOGEE, 5] = 85000.0                # APOGEE_HIGH
    summ[R.APOGEE, 6] = 50.0                   # APOGEE_LOW
    summ[R.RANGE, 7] = 250000.0                # RANGE
    summ[R.FLIGHT_TIME, 8] = 601.0             # FLIGHT_TIME
    summ[R.APOGEE, 9] = 79000.0                # valid: below every bound (ENERGY is 88 km)
    status[10] |= _abi.ST_NAN
    status[11] |= _abi.ST_INCOMPLETE
    summ[15, 12] = np.nan                      # a non-finite value of another row in a valid sample
    summ[R.IMPACT_X, 13] = np.inf              # a non-finite miss distance in a valid sample
    summ[2, 14] = -0.0
    return summ, status


def limit_state_specs():
    """(name, spec, kwargs of subset_ref.limit_state)."""
    out = []
    for name, row, tail, centre in (("range-upper", "range", "upper", None), ("row15-upper", 15, "upper", None),
                                    ("apogee-lower", "apogee_altitude", "lower", None), ("row2-lower", 2, "lower", None),
                                    ("miss", "range", "upper", (1500.0, -250.0)), ("miss-lower", "range", "lower", (0.0, 0.0))):
        spec = analysis.subset_spec(row=row, tail=tail, centre=centre)
        out.append((name, spec, {"row": spec.row, "sign": spec.sign, "centre": centre}))
    # a tighter energy bound: the ENERGY bit alone
    spec = analysis.subset_spec(bounds={"energy_apogee": 60000.0})
    out.append(("energy", spec, {"row": spec.row, "sign": 1, "centre": None, "bounds": BOUNDS[:4] + (60000.0,)}))
    return out


# ---- the whole run on the linear limit state: R = 24, 22 normal rows of weight 1 / sqrt(22), 2 uniform rows g ignores
LINEAR_KINDS = (1,) * 22 + (0,) * 2
LINEAR_CHAINS, LINEAR_STEPS, LINEAR_RHO = 512, 8, 0.8
LINEAR_TARGETS = ((4.7534, 1.0001e-6, 0.18, 11), (3.0902, 1.0001e-3, 0.106, 12))   # target, exact P, sized cov, seed
LINEAR_WEIGHT = 1.0 / math.sqrt(22.0)


def linear_draws0(seed):
    """Level 0 of the linear case: the independent draws of erpl_mc_design at `seed`, normal rows by the exact quantile."""
    import design_ref
    from scipy import special
    p, _ = design_ref.design(seed, design_ref.RANDOM, 24, LINEAR_CHAINS * LINEAR_STEPS)
    x = p.copy()
    x[:22] = special.ndtri(p[:22])
    return x


def linear_g(x):
    """Sum of the 22 normal rows in row order, times 1 / sqrt(22): the order every implementation of the test uses."""
    acc = x[0].copy()
    for r in range(1, 22):
        acc = acc + x[r]
    return acc * LINEAR_WEIGHT


def check_linear(out, exact, sized_cov):
    ratio = abs(math.log(out["probability"] / exact)) / out["cov"]
    assert ratio <= 4.0, (out["probability"], out["cov"], ratio)
    assert 0.5 * sized_cov <= out["cov"] <= 2.0 * sized_cov, out["cov"]
    return ratio
