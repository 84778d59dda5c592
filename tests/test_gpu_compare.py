"""erpl_mc_compare on the device against the NumPy yardstick of compare_ref.py: what has to hold exactly (counts, the integer
statistics K and 2 U_A of the observed labelling and of EVERY permutation, the location and sign of K, the quantiles, and with
them `exceed` of the two integer tests), the floating-point statistics T and E against an extended-precision truth, the
decisions on three pairs of clouds that the yardstick decided first (tests/test_compare_abi.py), the contracts of the call, and
one real pair of runs.

The floating-point tolerance is MEASURED, not fixed.  Truth is the exact rational (T) or the np.longdouble sum (E); the same
formulas are evaluated in plain float64 NumPy, and over the observed value and every replicate of a case the device's worst
relative error may be at most 4 x NumPy's worst plus (N + 64) 2^-53 for its sequential sums.  Every case prints both figures
(pytest -s)."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import compare_cases as cases
import compare_ref as ref
import helpers as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
R0, R1 = _abi.SUM_APOGEE_ALT, _abi.SUM_RANGE
RX, RY = _abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y
TILE = 256                                  # ERPL_CMP_TILE: members per workgroup of the pair pass, sources per LDS stage
SIZES = (2, 255, 256, 257, 1023, 1025, 2 * TILE + 3)
PERMS = (0, 1, 63, 64, 65, 200)
KINDS = ("continuous", "tied", "equal")
Q = (0.05, 0.25, 0.5, 0.75, 0.95)


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


def dev(engine, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def values(kind, m, rng, shift=0.0):
    """Two rows of m values: continuous, heavily tied (one decimal; both zeros occur) or all equal."""
    if kind == "equal":
        return np.full(m, 3.25), np.full(m, -0.0)
    a, b = rng.normal(shift, 1.0, m), rng.normal(0.0, 2.0, m) + shift
    if kind == "tied":
        a, b = np.round(a, 1), np.round(b, 1) * rng.choice([1.0, -1.0], m)     # -0.0 next to +0.0
    return a, b


def summary_of(cols, junk=False, seed=0):
    """(summary [16, n], mask [n] or None) of one run: `cols` maps a summary row to its m counted values.  With junk the m
    members are interleaved, in their order, with masked samples and with NaN / +-inf entries in any of the rows (the pattern
    of test_gpu_density.summary_of)."""
    rows = list(cols)
    m = len(cols[rows[0]])
    if not junk:
        summ = np.zeros((_abi.SUMMARY_DIM, m))
        for r in rows:
            summ[r] = cols[r]
        return summ, None
    rng = np.random.default_rng(seed + 77)
    n = m + max(7, m // 3)
    at = np.sort(rng.choice(n, size=m, replace=False))
    summ = np.zeros((_abi.SUMMARY_DIM, n))
    for r in rows:
        summ[r] = rng.normal(0.0, 1e4, n)                 # what a wrong population would pick up
    mask = np.zeros(n, dtype=np.uint8)
    for k, i in enumerate(np.setdiff1d(np.arange(n), at)):
        how, r = k % 5, rows[k % len(rows)]
        if how == 0:
            mask[i] = 1 + k % 63
        elif how == 1:
            summ[r, i] = np.nan
        elif how == 2:
            summ[r, i] = np.inf
        elif how == 3:
            summ[r, i] = -np.inf
            mask[i] = 4
        else:
            summ[rows[-1 - k % len(rows)], i] = np.nan
    for r in rows:
        summ[r, at] = cols[r]
    return summ, mask


def make_pair(kind, m_a, m_b, junk, seed):
    rng = np.random.default_rng(seed)
    a0, a1 = values(kind, m_a, rng)
    b0, b1 = values(kind, m_b, rng, shift=0.15)
    xa, ya, xb, yb = rng.normal(100.0, 30.0, m_a), rng.normal(-50.0, 10.0, m_a), rng.normal(104.0, 30.0, m_b), rng.normal(-50.0, 12.0, m_b)
    A = {R0: a0, R1: a1, RX: xa, RY: ya}
    B = {R0: b0, R1: b1, RX: xb, RY: yb}
    return A, B, summary_of(A, junk, seed), summary_of(B, junk, seed + 1)


def run(engine, sa, sb, **kw):
    (summ_a, mask_a), (summ_b, mask_b) = sa, sb
    kw.setdefault("rows", (R0, R1))
    kw.setdefault("quantiles", Q)
    return engine.compare(dev(engine, summ_a), dev(engine, summ_b), mask_a=dev(engine, mask_a), mask_b=dev(engine, mask_b), **kw)


def rel(got, truth):
    truth = np.asarray(truth, dtype=ref.LD)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64).astype(ref.LD) - truth) / np.maximum(np.abs(truth), ref.LD(1e-300))))


# Seeds are frozen per (N, P): the default is 1000 N + P; where that seed gives a permutation whose T or E ties with the observed
# value in exact arithmetic (a side of one member has only N labellings), the bracket of `exceed` is wider than 1 for any
# tolerance, and the case takes the next seed 10^6 k + 1000 N + P that does not.  Found on the CPU with the yardstick alone
# (the tolerance of a case is known without the device: 4 x NumPy's error + (N + 64) 2^-53).
BUMP = {(256, 64): 1}


def build_case(N, iN, P, iP, bump=None):
    """The inputs of one case and their yardstick."""
    kind, junk = KINDS[(iN + iP) % 3], bool((iN + iP // 3) % 2)
    m_a = max(1, (1, N // 3, N // 2)[iP % 3]) if N > 2 else 1
    m_b = N - m_a
    seed = 1000 * N + P + 10 ** 6 * (BUMP.get((N, P), 0) if bump is None else bump)
    A, B, sa, sb = make_pair(kind, m_a, m_b, junk, seed)
    truth = ref.compare([A[R0], A[R1]], [B[R0], B[R1]], (A[RX], A[RY]), (B[RX], B[RY]), permutations=P, seed=seed)
    return kind, junk, m_a, m_b, seed, A, B, sa, sb, truth


def brackets(truth, N, kind):
    """Per row j and for the energy statistic ('E'): the tolerance of the case and the bracket (lo, hi) of `exceed`."""
    out = {}
    for key, true, f64 in [(j, [s["T"] for s in st], [s["T64"] for s in st]) for j, st in enumerate(truth["rows"])] + \
            [("E", [s["E"] for s in truth["energy"]], [s["E64"] for s in truth["energy"]])]:
        tau = 4.0 * rel(f64, true) + (N + 64) * U
        obs, null = true[0], np.array(true[1:], dtype=ref.LD)
        out[key] = (tau, int(np.sum(null > obs * (1 + ref.LD(tau)))), int(np.sum(null >= obs * (1 - ref.LD(tau)))))
    return out


def narrow(truth, N, kind):
    """The brackets that have to be at most 1 wide: E always, T of continuous values, from N = 255 on."""
    b = brackets(truth, N, kind)
    keys = (["E"] + ([0, 1] if kind == "continuous" else [])) if N >= 255 else []
    return all(b[k][2] - b[k][1] <= 1 for k in keys)


def check_case(engine, N, iN, P, iP):
    """One call against the yardstick: everything exact, everything floating-point, and the brackets of `exceed`."""
    kind, junk, m_a, m_b, seed, A, B, sa, sb, truth = build_case(N, iN, P, iP)
    out = run(engine, sa, sb, permutations=P, seed=seed, keep_null=P > 0)
    label = f"N = {m_a} + {m_b}, P = {P}, {kind}{', junk' if junk else ''}"
    assert (out["count_a"], out["count_b"]) == (m_a, m_b), label
    assert out["n_a"] == sa[0].shape[1] and out["count_a"] + out["n_masked_a"] + out["n_non_finite_a"] == out["n_a"], label
    assert out["count_b"] + out["n_masked_b"] + out["n_non_finite_b"] == out["n_b"], label
    null = out["null_values"].cpu().numpy() if P > 0 else np.zeros((7, 0))
    # the device's labels are the host's, and the host's are the yardstick's
    if P > 0:
        assert np.array_equal(analysis.permutation_labels(seed, P - 1, m_a, m_b), truth["labels"][P]), label
    assert P == 0 or narrow(truth, N, kind), (label, "the bracket of the case is too wide: choose another seed")
    tau = {}
    for j, r in enumerate((R0, R1)):
        row, st = out["row"][j], truth["rows"][j]
        obs = st[0]
        assert (row["ks_num"], row["u2_a"], row["ks_sign"]) == (obs["K"], obs["U2"], obs["sign"]), (label, r)
        assert row["ks_at"] == obs["value"] and row["ks"]["statistic"] == obs["D"] and row["mw"]["statistic"] == float(obs["mw"]), (label, r)
        assert row["prob_superiority"] == obs["U2"] / ((2.0 * m_a) * m_b), (label, r)
        for k, q in enumerate(Q):
            qa, qb = ref.quantile(A[r], q), ref.quantile(B[r], q)
            assert (row["quantile_a"][k], row["quantile_b"][k], row["shift"][k]) == (qa, qb, qb - qa), (label, r, q)
        assert abs(row["mean_a"] - np.mean(A[r])) <= 1e-12 * max(1.0, abs(np.mean(A[r]))) and abs(row["std_b"] - np.std(B[r])) <= 1e-12 * max(1.0, np.std(B[r]))
        if kind == "equal":
            assert row["ks_num"] == 0 and row["ks_sign"] == 0 and row["ks"]["statistic"] == 0.0, (label, r)
        t_true = [s["T"] for s in st]
        t_dev = np.r_[row["cvm"]["statistic"], null[3 * j + 2]]
        e_np, e_dev = rel([s["T64"] for s in st], t_true), rel(t_dev, t_true)
        tau[j] = 4.0 * e_np + (N + 64) * U
        print(f"{label} row {r}: T rel. error NumPy {e_np:.3g}, device {e_dev:.3g}, bound {tau[j]:.3g}")
        assert e_dev <= tau[j], (label, r)
        if P == 0:
            for key in ("ks", "mw", "cvm"):
                assert row[key]["exceed"] == 0 and all(np.isnan(row[key][f]) for f in ("p_value", "null_mean", "null_hi")), (label, r)
            continue
        assert np.array_equal(null[3 * j], [float(s["K"]) for s in st[1:]]), (label, r)
        assert np.array_equal(null[3 * j + 1], [float(s["U2"]) for s in st[1:]]), (label, r)
        for key, name in (("ks", "K"), ("mw", "mw")):
            want = ref.null_summary([s[name] for s in st[1:]], obs[name], 0.95)
            assert row[key]["exceed"] == want["exceed"] and row[key]["p_value"] == want["p"], (label, r, key)
        if kind == "equal":
            assert row["ks"]["p_value"] == 1.0 and row["cvm"]["exceed"] == P, (label, r)
        assert row["ks"]["null_hi"] == np.quantile([s["K"] / (float(m_a) * m_b) for s in st[1:]], 0.95), (label, r)
        t_obs, t_null = t_true[0], np.array(t_true[1:])
        lo, hi = int(np.sum(t_null > t_obs * (1 + ref.LD(tau[j])))), int(np.sum(t_null >= t_obs * (1 - ref.LD(tau[j]))))
        assert lo <= row["cvm"]["exceed"] <= hi, (label, r, lo, row["cvm"]["exceed"], hi)
    e = out["energy"]
    en = truth["energy"]
    e_true = [s["E"] for s in en]
    e_dev = np.r_[e["statistic"], null[6]]
    e_np, e_devr = rel([s["E64"] for s in en], e_true), rel(e_dev, e_true)
    bound = 4.0 * e_np + (N + 64) * U
    print(f"{label}: E rel. error NumPy {e_np:.3g}, device {e_devr:.3g}, bound {bound:.3g}")
    assert e_devr <= bound, label
    # the mean distances: sums of positive terms, (N + 64) 2^-53 for a sequential sum; d_bb comes from t_i - r_i, which the
    # splits of this table (m_b >= N / 2) amplify by N / m_b <= 2, once per member and once in the sum over the members
    for key in ("d_aa", "d_ab", "d_bb"):
        assert abs(e[key] - float(en[0][key])) <= 4 * (N + 64) * U * float(en[0][key]), (label, key)
    if P > 0:
        e_obs, e_null = e_true[0], np.array(e_true[1:])
        lo, hi = int(np.sum(e_null > e_obs * (1 + ref.LD(bound)))), int(np.sum(e_null >= e_obs * (1 - ref.LD(bound))))
        assert lo <= e["exceed"] <= hi, (label, lo, e["exceed"], hi)
        assert e["p_value"] == (e["exceed"] + 1) / (P + 1), label


@pytest.mark.parametrize("iN", range(len(SIZES)), ids=[f"N{n}" for n in SIZES])
def test_exact_and_floating_point_against_the_yardstick(engine, iN):
    """Pooled N over the sizes of the issue, every P of the issue per size; the split (1 : N - 1, 1 : 2, equal), the kind of
    values (continuous, heavily tied, all equal) and junk in the inputs rotate through the (N, P) grid so that every value of
    each occurs with every N and every P range."""
    for iP, P in enumerate(PERMS):
        check_case(engine, SIZES[iN], iN, P, iP)


def test_it_decides_correctly(engine):
    """1500 against 1000 bivariate normal points, P = 999, the cases the yardstick decided in tests/test_compare_abi.py:
    (a) the same law: every p > 0.05; (b) the mean of x moved by 0.3 sigma: KS, CvM, Mann-Whitney of x and the energy test at
    p = 1 / 1000; (c) the same marginals, correlation + 0.5 against - 0.5: the energy test at 1 / 1000, every rank test
    above 0.05."""
    for name in ("same", "shift", "corr"):
        xa, ya, xb, yb = cases.law(name)
        out = run(engine, summary_of({RX: xa, RY: ya}), summary_of({RX: xb, RY: yb}), rows=(RX, RY), permutations=cases.DECISION_P,
                  seed=cases.DECISION_SEED)
        p = [out["row"][j][k]["p_value"] for j in range(2) for k in ("ks", "mw", "cvm")]
        pe = out["energy"]["p_value"]
        print(name, p, pe, out["energy"]["statistic"], out["energy"]["null_hi"])
        if name == "same":
            assert min(p + [pe]) > 0.05
        elif name == "shift":
            assert p[:3] == [0.001] * 3 and pe == 0.001
        else:
            assert pe == 0.001 and min(p) > 0.05


def test_contracts(engine):
    A, B, sa, sb = make_pair("tied", 700, 325, True, 5)
    base = run(engine, sa, sb, permutations=65, seed=9, keep_null=True)
    # two calls, another stream, an unrelated call in between: the same bytes
    engine.bootstrap(dev(engine, sa[0]), dev(engine, sa[1]), rows=(R0,), replicates=8)
    with torch.cuda.stream(torch.cuda.Stream(engine.device)):
        again = run(engine, sa, sb, permutations=65, seed=9, keep_null=True)
        torch.cuda.current_stream(engine.device).synchronize()
    assert torch.equal(base["null_values"].view(torch.int64), again["null_values"].view(torch.int64))
    strip = lambda o: {k: v for k, v in o.items() if k not in ("null_values", "ecdf", "cloud_a", "cloud_b")}   # noqa: E731
    assert H.same_nested(strip(base), strip(again))
    # swapping the runs mirrors the result
    swapped = run(engine, sb, sa, permutations=0)
    m_a, m_b = base["count_a"], base["count_b"]
    for j in range(2):
        r, s = base["row"][j], swapped["row"][j]
        assert (s["ks_num"], s["ks_sign"], s["ks_at"]) == (r["ks_num"], -r["ks_sign"], r["ks_at"])
        assert s["u2_a"] == 2 * m_a * m_b - r["u2_a"] and s["cvm"]["statistic"] == r["cvm"]["statistic"]
        assert s["mw"]["statistic"] == r["mw"]["statistic"] and s["quantile_a"] == r["quantile_b"]
    assert abs(swapped["energy"]["statistic"] - base["energy"]["statistic"]) <= (m_a + m_b + 64) * U * base["energy"]["d_ab"]
    assert swapped["energy"]["d_aa"] == pytest.approx(base["energy"]["d_bb"], rel=1e-13)
    # P = 0: nothing depends on the seed
    one, two = strip(run(engine, sa, sb, permutations=0, seed=1)), strip(run(engine, sa, sb, permutations=0, seed=2 ** 63))
    assert (one.pop("seed"), two.pop("seed")) == (1, 2 ** 63) and H.same_nested(one, two)
    # row_x = -1: the rank results of the full call, where the populations coincide (clean inputs)
    clean = make_pair("continuous", 300, 400, False, 6)
    full, ranks = run(engine, clean[2], clean[3], permutations=65, seed=3), run(engine, clean[2], clean[3], permutations=65, seed=3, xy=None)
    assert ranks["energy"] is None and H.same_nested(full["row"], ranks["row"])


def test_energy_limit_and_empty_sides(engine):
    n = 40000
    big = torch.zeros((_abi.SUMMARY_DIM, n), dtype=torch.float64, device=engine.device)
    with pytest.raises(_abi.ErplError, match="spec->row_x = -1 runs the rank tests alone"):
        engine.compare(big, big, permutations=0)
    half = torch.zeros(n, dtype=torch.uint8, device=engine.device)
    half[n // 4:] = 1
    out = engine.compare(big, big, mask_a=half, mask_b=half, permutations=0)      # 10 000 + 10 000 pooled points: runs
    assert (out["count_a"], out["count_b"]) == (n // 4, n // 4) and out["energy"]["statistic"] == 0.0
    assert engine.compare(big, big, xy=None, permutations=1)["row"][0]["ks"]["p_value"] == 1.0    # the rest runs at any size
    nothing = torch.ones(n, dtype=torch.uint8, device=engine.device)
    out = engine.compare(big, big, mask_a=nothing, permutations=7, keep_null=True)
    assert (out["count_a"], out["count_b"]) == (0, n) and out["energy"] is None
    assert np.isnan(out["row"][0]["ks"]["statistic"]) and np.isnan(out["row"][0]["mean_a"]) and out["row"][0]["mean_b"] == 0.0
    assert out["row"][0]["ks_num"] == 0 and bool(torch.isnan(out["null_values"]).all())
    both = engine.compare(big, big, mask_a=nothing, mask_b=nothing, permutations=0)
    assert (both["count_a"], both["count_b"]) == (0, 0) and np.isnan(both["row"][1]["cvm"]["statistic"])


@pytest.fixture(scope="module")
def real_runs():
    """4096 f64_fast flights of run_monte_carlo_device; the same with another seed; the same seed with the launch elevation
    moved by 0.005 rad, the sigma of the initial attitude in the reference's uncertainty table (monte_carlo.py:38).

    The flights are those of the in-plane dispersion (planar=True, Set P), the set whose vehicles fly: the outlier filter keeps
    about 3300 of 4096.  Under the default dispersion model nearly every vehicle tumbles and the filter keeps
    100 of 4096; the range of those is the range of tumbling vehicles (standard deviation 11 km) and says nothing about the
    launch elevation: there the same move shifts it by 0.05 sigma, p = 0.878 / 0.911 / 0.935 (measured on an MI355X)."""
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    an = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    ic = dict(H.EXAMPLE_IC)
    moved_ic = dict(ic, attitude=[ic["attitude"][0], ic["attitude"][1] + H.UNCERTAINTY["initial_attitude"][1], ic["attitude"][2]])
    return an, {"base": an.run_monte_carlo_device(ic, 4096, seed=1234, precision="f64_fast", planar=True),
                "seed": an.run_monte_carlo_device(ic, 4096, seed=4321, precision="f64_fast", planar=True),
                "moved": an.run_monte_carlo_device(moved_ic, 4096, seed=1234, precision="f64_fast", planar=True)}


def test_one_real_pair_another_seed_does_not_reject(real_runs):
    """Against 4096 flights with another seed no test rejects at 0.01 (the filtered populations: 3292 against 3308 flights;
    measured: the smallest p of the nine rank tests 0.141, the energy test 0.879)."""
    an, runs = real_runs
    same = an.compare_runs(runs["base"], runs["seed"], permutations=999, seed=1)
    print([r["verdict"] for r in same["row"]], same["energy_verdict"], same["count_a"], same["count_b"])
    assert [r["name"] for r in same["row"]] == ["apogee_altitude", "range", "flight_time"]
    assert 2048 < same["count_a"] <= same["n_samples_a"] and 2048 < same["count_b"] <= same["n_samples_b"]
    assert min(min(r["p_values"].values()) for r in same["row"]) > 0.01 and same["energy"]["p_value"] > 0.01
    assert all("no difference at 0.05" in r["verdict"] for r in same["row"] if min(r["p_values"].values()) > 0.05)


def test_one_real_pair_moved_elevation_rejects_on_range(real_runs):
    """Against the same seed with the launch elevation moved by 0.005 rad range rejects at 0.01 in all three tests (measured:
    3292 against 3371 kept flights, the range moves by + 411 m against a standard deviation of 1429 m, every p = 1 / 1000, the
    energy test of the impact clouds as well; apogee and flight time stay above 0.5)."""
    an, runs = real_runs
    diff = an.compare_runs(runs["base"], runs["moved"], permutations=999, seed=1)
    print([r["verdict"] for r in diff["row"]], diff["energy_verdict"], diff["count_a"], diff["count_b"])
    assert max(diff["row"][1]["p_values"].values()) <= 0.01
    assert "differs" in diff["row"][1]["verdict"] and diff["energy"]["p_value"] <= 0.01


def test_permutations_in_blocks(engine):
    """300 000 + 300 000 members and P = 4096: 65 words of label bits per member are 312 MB, more than the 256 MiB the layout
    allows, so the permutations run in two blocks (55 and 10 words: replicates 0 .. 3519 and 3520 .. 4096).  The observed
    statistics and the permutations at both ends of both blocks against the yardstick (values rounded to three decimals:
    ties), and `exceed` consistent with the null values the call returns."""
    m, P, seed = 300000, 4096, 77
    rng = np.random.default_rng(seed)
    a, b = np.round(rng.normal(size=m), 3), np.round(rng.normal(0.004, 1.0, size=m), 3)
    out = run(engine, summary_of({R0: a}), summary_of({R0: b}), rows=(R0,), xy=None, permutations=P, seed=seed, keep_null=True)
    assert (out["count_a"], out["count_b"]) == (m, m) and (256 << 20) // (8 * 2 * m) == 55
    null, row = out["null_values"].cpu().numpy(), out["row"][0]
    rk = ref.Ranked(np.r_[a, b])
    obs = ref.rank_stats(rk, ref.identity(m, m))
    assert (row["ks_num"], row["u2_a"], row["ks_sign"], row["ks_at"]) == (obs["K"], obs["U2"], obs["sign"], obs["value"])
    assert abs(row["cvm"]["statistic"] - float(obs["T"])) <= 4 * U * float(obs["T"])
    for p in (0, 3518, 3519, 4095):          # replicate p + 1: the last of block 0 is 3519, the first of block 1 is 3520
        st = ref.rank_stats(rk, ref.labels(seed, p, m, m))
        assert (null[0, p], null[1, p]) == (float(st["K"]), float(st["U2"])), p
        assert abs(null[2, p] - float(st["T"])) <= 4 * U * float(st["T"]), p
    assert row["ks"]["exceed"] == int(np.sum(null[0] >= row["ks_num"])) and row["cvm"]["exceed"] == int(np.sum(null[2] >= row["cvm"]["statistic"]))
    assert row["mw"]["exceed"] == int(np.sum(np.abs(null[1] - float(m) * m) >= row["mw"]["statistic"]))
    # K = m |c_A - c_B| at equal sizes, |c_A - c_B| a few hundred: hundreds of distinct values, not one per permutation
    assert len(np.unique(null[0])) > 100 and row["ks"]["p_value"] == (row["ks"]["exceed"] + 1) / (P + 1)
