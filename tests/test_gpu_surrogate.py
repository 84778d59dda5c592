"""erpl_mc_surrogate and erpl_mc_surrogate_predict on the device against the NumPy restatement of surrogate_ref on host copies
of the same tensors.

Equal: the counts and the terms.  Equal to the bit: the device's predictions, those of erpl_mc_surrogate_predict_host and
surrogate_ref's (the same operations in the same order, no contraction), NaN for a non-finite input, the columns from n on
untouched; every output of two calls; the outputs when the masked-out samples hold garbage or masked samples are appended.
Gram and right-hand sides: |device - NumPy| <= 2 gamma_{m+1} (|Psi| |Psi|^T), m = n_fit, gamma_k = k u / (1 - k u), u = 2^-53:
either side is a sum of m products in SOME order (fused or not), each within gamma_{m+1} (|Psi| |Psi|^T) of the exact
sum, whatever the order (Higham, Accuracy and Stability, section 3.1) - nothing in it is tuned to the device.  Symmetry exact.
Solve, on the device's own G and b in long double: ||b - G c||_2 <= P gamma_{3P+1} ||G||_2 ||c||_2 (Higham, theorem 10.4: the
backward error of a Cholesky solve is |dG| <= gamma_{3P+1} |R^T| |R|, and || |R^T| |R| ||_2 <= P ||G||_2); where the
reference's cond(G) <= 1e4 the coefficients are within cond(G) times that relative bound of the long double solution.
fit_ok is 1 wherever n_fit >= 2 P.  What is derived - r2, q2, tss, rss, mean, variance_pce, first, total, pair - against
surrogate_ref evaluated from the RETURNED coefficients: 1e-12 relative (the bar of test_gpu_bootstrap.py), nothing added."""
import ctypes as C

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, models

import helpers as H
import surrogate_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-12
UNIT = 2.0 ** -53
EXTRA = _abi.SUR_ROW_EXTRA
ROWS = [_abi.SUM_FIRST_APOGEE_ALT, EXTRA, _abi.SUM_RANGE]
# (members, n_vars, degree, order, holdout)
# the last one: 276 terms, 3 tiles a side; its chunk of 21 760 fitted members is cut into 85 slices where a chunk of the
# layout's own length (21 776) has 81 - the partial tiles must hold the 85
CASES = [(1, 1, 1, 1, 0), (63, 1, 12, 1, 0), (64, 3, 2, 2, 2), (65, 3, 2, 2, 0), (255, 2, 12, 2, 0), (257, 5, 4, 3, 3),
         (1200, 32, 2, 2, 0), (2000, 25, 3, 2, 5), (1000, 32, 12, 1, 0), (4099, 3, 12, 3, 7), (70001, 4, 3, 2, 0),
         (21760, 22, 2, 2, 0)]
DIRTY = 9      # samples outside the population: 3 masked, 6 not finite


def gamma(k):
    return k * UNIT / (1.0 - k * UNIT)


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


def dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def make_inputs(case):
    """factors [V, n] (even rows normal, odd rows uniform), a [16, n] summary, an extra row and a mask with n = members + 9:
    three samples masked (one of them with a NaN row as well: counted as masked), a NaN and an infinity in a variable, a NaN
    and an infinity in the summary rows, an infinity and a NaN in `extra`.  The rows are smooth functions of the variables
    plus 5 % noise, so that r2 and q2 are of order one."""
    m, V, degree, order, holdout = case
    n = m + DIRTY
    rng = np.random.default_rng(1000 * m + V)
    kinds = [_abi.DESIGN_NORMAL if v % 2 == 0 else _abi.DESIGN_UNIFORM for v in range(V)]
    fac = np.vstack([rng.normal(size=n) if k == _abi.DESIGN_NORMAL else rng.uniform(size=n) for k in kinds])
    t = np.vstack([fac[v] if k == _abi.DESIGN_NORMAL else 2.0 * fac[v] - 1.0 for v, k in enumerate(kinds)])
    summ = rng.normal(size=(_abi.SUMMARY_DIM, n))
    extra = np.empty(n)
    for j, r in enumerate(ROWS):
        y = 3.0 + j + rng.normal(size=V) @ t + 0.3 * (rng.normal(size=V) @ t ** 2) + 0.4 * t[0] * t[V - 1] + 0.05 * rng.normal(size=n)
        if r == EXTRA:
            extra[:] = y
        else:
            summ[r] = y
    mask = np.zeros(n, dtype=np.uint8)
    where = rng.permutation(n)[:DIRTY]
    mask[where[:3]] = [1, 4, 32]
    fac[0, where[3]], fac[V - 1, where[4]] = np.nan, np.inf
    summ[ROWS[0], where[5]], extra[where[6]], summ[ROWS[2], where[7]], extra[where[8]] = np.nan, -np.inf, np.inf, np.nan
    summ[ROWS[0], where[0]] = np.nan
    return kinds, fac, summ, extra, mask


def run(engine, case, kinds, fac, summ, extra, mask):
    _, V, degree, order, holdout = case
    return engine.surrogate(dev(engine, fac), kinds, dev(engine, summ), dev(engine, mask), rows=ROWS, extra=dev(engine, extra),
                            degree=degree, order=order, holdout=holdout, want_gram=True)


_cache = {}


def solved(engine, case):
    """The inputs of a case, the device's result and the reference's view of the same population, once per case."""
    if case not in _cache:
        kinds, fac, summ, extra, mask = make_inputs(case)
        out = run(engine, case, kinds, fac, summ, extra, mask)
        ys = np.vstack([extra if r == EXTRA else summ[r] for r in ROWS])
        members, fit, val, n_masked, n_bad = R.population(fac, ys, mask, case[4])
        tm = R.terms(case[1], case[2], case[3])
        _cache[case] = dict(kinds=kinds, fac=fac, summ=summ, extra=extra, mask=mask, out=out, ys=ys, members=members, fit=fit, val=val,
                            n_masked=n_masked, n_bad=n_bad, tm=tm, Psi=R.basis(kinds, fac[:, fit], tm, case[2]))
    return _cache[case]


def same_outputs(a, b, skip=("n", "n_masked")):
    for key in a:
        if key in skip:
            continue
        if key == "model":
            assert a[key]["terms"].tobytes() == b[key]["terms"].tobytes() and \
                a[key]["coefficients"].tobytes() == b[key]["coefficients"].tobytes(), key
        elif isinstance(a[key], np.ndarray):
            assert a[key].tobytes() == b[key].tobytes(), key
        elif isinstance(a[key], float):
            assert np.float64(a[key]).tobytes() == np.float64(b[key]).tobytes(), key
        else:
            assert a[key] == b[key], key


case_ids = ["-".join(map(str, c)) for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_counts_terms_and_predictions(engine, case):
    s = solved(engine, case)
    out, (m, V, degree, order, holdout) = s["out"], case
    assert (out["n"], out["count"], out["n_masked"], out["n_non_finite"]) == (m + DIRTY, m, 3, 6) == \
        (len(s["mask"]), len(s["members"]), s["n_masked"], s["n_bad"])
    assert (out["n_fit"], out["n_val"]) == (len(s["fit"]), len(s["val"])) and out["n_fit"] + out["n_val"] == m
    assert out["rows"] == ROWS and out["n_terms"] == len(s["tm"]) == R.count(V, degree, order)
    from erpl_monte_carlo_sim_amd import analysis
    assert np.array_equal(out["model"]["terms"], s["tm"]) and np.array_equal(analysis.surrogate_terms(V, degree, order), s["tm"])
    # predictions: the fitted model and one with random coefficients, at the run's own columns (NaN and inf among them);
    # ld = n + 5 with a sentinel behind the columns
    rng = np.random.default_rng(7)
    n = m + DIRTY
    X = np.hstack([s["fac"], rng.uniform(0.1, 0.9, size=(V, 5))])
    lib = H.load_lib()
    for coef in (out["model"]["coefficients"], rng.normal(size=(2, len(s["tm"])))):
        model = dict(out["model"], coefficients=coef)
        got = engine.surrogate_predict(model, dev(engine, X), out=torch.full((len(coef), n + 5), -7.0, dtype=torch.float64,
                                                                              device=engine.device), n=n).cpu().numpy()
        assert np.all(got[:, n:] == -7.0)
        want = R.predict(s["kinds"], degree, s["tm"], coef, X[:, :n])
        host = np.full((len(coef), n + 5), -7.0)
        spec = _abi.ErplSurSpec()
        spec.n_vars, spec.n_rows, spec.degree, spec.order = V, len(coef), degree, order
        coef_c = np.ascontiguousarray(coef, dtype=np.float64)
        assert lib.erpl_mc_surrogate_predict_host(C.byref(spec), bytes(s["kinds"]), C.c_void_p(coef_c.ctypes.data), C.c_void_p(X.ctypes.data),
                                                  n + 5, n, C.c_void_p(host.ctypes.data)) == 0
        bad = ~np.all(np.isfinite(X[:, :n]), axis=0)
        assert bad.sum() == 2 and np.all(np.isnan(got[:, :n][:, bad]))
        for other in (want, host[:, :n]):
            assert np.array_equal(np.isnan(got[:, :n]), np.isnan(other))
            assert np.all(np.isnan(other) | (got[:, :n].view(np.uint64) == other.view(np.uint64)))


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_gram_and_right_hand_sides_within_the_summation_bound(engine, case):
    s = solved(engine, case)
    out, Psi = s["out"], s["Psi"]
    G, b = out["gram"], out["rhs"]
    assert np.array_equal(G, G.T)
    g = 2.0 * gamma(len(s["fit"]) + 1)
    y = s["ys"][:, s["fit"]]
    bound_G, bound_b = g * (np.abs(Psi) @ np.abs(Psi).T), g * (np.abs(y) @ np.abs(Psi).T)
    share_G = np.max(np.abs(G - Psi @ Psi.T) / bound_G)
    share_b = np.max(np.abs(b - y @ Psi.T) / bound_b)
    print(f"{case}: worst share of the bound: gram {share_G:.3f}, rhs {share_b:.3f}")
    assert share_G <= 1.0 and share_b <= 1.0


def cholesky_solve_long(G, B):
    """G c = b for every row b of B in long double: right-looking Cholesky, two triangular solves."""
    A = np.array(G, dtype=np.longdouble)
    P = len(A)
    for j in range(P):
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    L = np.tril(A)
    out = np.empty((len(B), P), dtype=np.longdouble)
    for r, b in enumerate(np.asarray(B, dtype=np.longdouble)):
        z = np.empty(P, dtype=np.longdouble)
        for i in range(P):
            z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
        c = np.empty(P, dtype=np.longdouble)
        for i in range(P - 1, -1, -1):
            c[i] = (z[i] - L[i + 1:, i] @ c[i + 1:]) / L[i, i]
        out[r] = c
    return out


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_solve_within_the_bound_of_a_cholesky_solve(engine, case):
    s = solved(engine, case)
    out = s["out"]
    P, n_fit = out["n_terms"], out["n_fit"]
    coef = out["model"]["coefficients"]
    if n_fit < P:
        assert not out["fit_ok"].any()
    if n_fit >= 2 * P:
        assert out["fit_ok"].all()
    assert out["fit_ok"].all() or not out["fit_ok"].any()      # one factorisation serves every row
    if not out["fit_ok"].any():     # still ERPL_OK: the coefficients and what is derived from them are NaN
        assert np.all(np.isnan(coef)) and np.all(np.isnan(out["r2"])) and np.all(np.isnan(out["first"])) and np.all(np.isnan(out["total"]))
        assert np.all(np.isnan(out["pair"])) and np.all(np.isnan(out["mean"])) and np.all(np.isnan(out["variance_pce"]))
        assert np.all(np.isfinite(out["tss_fit"]))
        return
    assert 0.0 < out["pivot_min"] <= out["pivot_max"] < np.inf
    G, b = out["gram"].astype(np.longdouble), out["rhs"].astype(np.longdouble)
    norm_G = float(np.max(np.abs(np.linalg.eigvalsh(out["gram"]))))
    rel = P * gamma(3 * P + 1)
    eig = np.linalg.eigvalsh(s["Psi"] @ s["Psi"].T)
    cond = float(eig[-1] / eig[0]) if eig[0] > 0 else np.inf
    exact = cholesky_solve_long(out["gram"], out["rhs"]) if cond <= 1e4 else None
    for j in range(len(ROWS)):
        c = coef[j].astype(np.longdouble)
        res = float(np.sqrt(np.sum((b[j] - G @ c) ** 2)))
        bound = rel * norm_G * float(np.sqrt(np.sum(c * c)))
        print(f"{case} row {j}: residual {res:.3e} = {res / bound:.4f} of the bound, cond {cond:.3e}")
        assert res <= bound
        if exact is not None:
            err = float(np.sqrt(np.sum((c - exact[j]) ** 2))) / float(np.sqrt(np.sum(exact[j] ** 2)))
            assert err <= cond * rel, (err, cond * rel)


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = np.isnan(want) | (np.abs(got - want) <= TOL * np.abs(want))
    assert np.all(ok), (got, want)


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_derived_values_from_the_returned_coefficients(engine, case):
    s = solved(engine, case)
    out, (m, V, degree, order, holdout) = s["out"], case
    coef = out["model"]["coefficients"]
    yhat = R.predict(s["kinds"], degree, s["tm"], coef, s["fac"])
    for j in range(len(ROWS)):
        y = s["ys"][j]
        tss, rss, r2 = R.residuals(y[s["fit"]], yhat[j, s["fit"]])
        close(out["tss_fit"][j], tss)
        close(out["rss_fit"][j], rss)
        close(out["r2"][j], r2)
        tss, rss, q2 = R.residuals(y[s["val"]], yhat[j, s["val"]])
        close(out["tss_val"][j], tss)
        close(out["rss_val"][j], rss)
        close(out["q2"][j], q2)
        if holdout == 0:
            assert np.isnan(out["tss_val"][j]) and np.isnan(out["q2"][j]) and out["n_val"] == 0
        if not out["fit_ok"][j]:
            continue
        mean, var, first, total, pair = R.derived(coef[j], s["tm"], V)
        close(out["mean"][j], mean)
        close(out["variance_pce"][j], var)
        close(out["first"][j], first)
        close(out["total"][j], total)
        close(out["pair"][j], pair)
        assert np.array_equal(out["pair"][j], out["pair"][j].T) and np.all(np.diag(out["pair"][j]) == 0.0)
        if n_rich(out):
            assert 0.5 < out["r2"][j] <= 1.0      # the rows are smooth in the variables: a fit that explains nothing is wrong


def n_rich(out):
    return out["n_fit"] >= 4 * out["n_terms"]


def test_a_constant_row_has_nan_r2_and_nan_indices(engine):
    case = (65, 3, 2, 2, 2)
    kinds, fac, summ, extra, mask = make_inputs(case)
    extra[np.isfinite(extra)] = 7.25
    out = run(engine, case, kinds, fac, summ, extra, mask)
    assert out["fit_ok"].all() and out["tss_fit"][1] == 0.0 and out["tss_val"][1] == 0.0
    assert np.isnan(out["r2"][1]) and np.isnan(out["q2"][1]) and np.isfinite(out["r2"][0]) and np.isfinite(out["q2"][2])
    assert abs(out["mean"][1] - 7.25) <= 1e-9


def test_a_zero_row_has_zero_variance_and_nan_indices(engine):
    """A row of zeros: b = 0 exactly, so the solve returns zeros exactly (0 / pivot, and 0 - l 0 = 0), variance_pce == 0 and
    the rule for it holds on the device's own result, whatever the rounding of G: every index NaN, pair included; the other
    rows are untouched."""
    case = (65, 3, 2, 2, 2)
    kinds, fac, summ, extra, mask = make_inputs(case)
    extra[np.isfinite(extra)] = 0.0
    out = run(engine, case, kinds, fac, summ, extra, mask)
    assert out["fit_ok"].all() and np.all(out["model"]["coefficients"][1] == 0.0) and np.all(out["rhs"][1] == 0.0)
    assert out["mean"][1] == 0.0 and out["variance_pce"][1] == 0.0 and out["tss_fit"][1] == 0.0 and out["rss_fit"][1] == 0.0
    assert np.all(np.isnan(out["first"][1])) and np.all(np.isnan(out["total"][1])) and np.all(np.isnan(out["pair"][1]))
    assert np.isnan(out["r2"][1]) and np.isnan(out["q2"][1])
    mean, var, first, total, pair = R.derived(out["model"]["coefficients"][1], R.terms(3, 2, 2), 3)
    assert var == 0.0 and np.all(np.isnan(first)) and np.all(np.isnan(total)) and np.all(np.isnan(pair))
    for j in (0, 2):
        assert np.all(np.isfinite(out["first"][j])) and np.all(np.isfinite(out["pair"][j])) and out["variance_pce"][j] > 0.0


def test_an_empty_population_is_ok_and_all_nan(engine):
    case = (65, 3, 2, 2, 2)
    kinds, fac, summ, extra, mask = make_inputs(case)
    out = run(engine, case, kinds, fac, summ, extra, np.full(len(mask), 8, dtype=np.uint8))
    assert (out["count"], out["n_fit"], out["n_val"], out["n_masked"], out["n_non_finite"]) == (0, 0, 0, len(mask), 0)
    assert not out["fit_ok"].any() and np.all(np.isnan(out["model"]["coefficients"])) and np.all(out["gram"] == 0.0) and np.all(out["rhs"] == 0.0)
    assert np.isnan(out["pivot_min"]) and np.isnan(out["pivot_max"])
    for key in ("mean", "variance_pce", "tss_fit", "rss_fit", "r2", "tss_val", "rss_val", "q2", "first", "total", "pair"):
        assert np.all(np.isnan(out[key])), key
    again = run(engine, case, kinds, fac, summ, extra, mask)      # and the context is as good as before
    assert again["count"] == 65 and again["fit_ok"].all()


def test_a_row_fitted_alone_or_among_three_has_the_same_bits(engine):
    """126 terms: one requested row makes the product 127 rows (one tile a side), three make it 129 (two).  The slices are cut
    from (n_fit, P) alone, so G, the row's b, its coefficients and everything derived from them are the same bytes."""
    case = (1500, 25, 5, 1, 0)
    kinds, fac, summ, extra, mask = make_inputs(case)
    for r in (ROWS[0], ROWS[2]):       # one population for both calls: only `extra` and the variables decide it
        summ[r, ~np.isfinite(summ[r])] = 1.0
    three = run(engine, case, kinds, fac, summ, extra, mask)
    alone = engine.surrogate(dev(engine, fac), kinds, dev(engine, summ), dev(engine, mask), rows=[EXTRA], extra=dev(engine, extra),
                             degree=5, order=1, holdout=0, want_gram=True)
    assert three["n_terms"] == alone["n_terms"] == 126 and three["count"] == alone["count"] == 1500 + DIRTY - 3 - 4
    assert three["fit_ok"].all() and alone["fit_ok"].all()
    assert three["gram"].tobytes() == alone["gram"].tobytes() and three["rhs"][1].tobytes() == alone["rhs"][0].tobytes()
    assert three["model"]["coefficients"][1].tobytes() == alone["model"]["coefficients"][0].tobytes()
    for key in ("mean", "variance_pce", "tss_fit", "rss_fit", "r2", "first", "total", "pair"):
        assert np.asarray(three[key][1]).tobytes() == np.asarray(alone[key][0]).tobytes(), key


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_repeatable_and_independent_of_what_is_outside_the_population(engine, case):
    s = solved(engine, case)
    kinds, fac, summ, extra, mask = s["kinds"], s["fac"], s["summ"], s["extra"], s["mask"]
    same_outputs(s["out"], run(engine, case, kinds, fac, summ, extra, mask), skip=())
    rng = np.random.default_rng(11)
    gone = mask != 0
    fac2, summ2, extra2 = fac.copy(), summ.copy(), extra.copy()
    fac2[:, gone] = rng.normal(size=(fac.shape[0], gone.sum())) * 1e30
    summ2[:, gone], extra2[gone] = np.nan, np.inf
    same_outputs(s["out"], run(engine, case, kinds, fac2, summ2, extra2, mask), skip=())
    k = 37
    grown = run(engine, case, kinds, np.hstack([fac, rng.normal(size=(fac.shape[0], k))]), np.hstack([summ, rng.normal(size=(16, k))]),
                np.concatenate([extra, rng.normal(size=k)]), np.concatenate([mask, np.full(k, 2, dtype=np.uint8)]))
    assert grown["n"] == s["out"]["n"] + k and grown["n_masked"] == s["out"]["n_masked"] + k
    same_outputs(s["out"], grown)


def test_a_lhs_flight_end_to_end(engine, tmp_path):
    """1 024 planar flights drawn as one Latin hypercube: the regenerated primitive rows are the flown window bit for bit, the
    fit succeeds, and predicting at the flown inputs reproduces r2 from its own residuals.  No threshold on r2 or q2."""
    from erpl_monte_carlo_sim_amd import sampling
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    run_ = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 1024, seed=99, planar=True, design="lhs")
    sur = mc.surrogate(run_, degree=2, order=2, holdout=4)
    K = 100
    flown = sampling.design_draws(1024, K, engine.device, 99, design="lhs")
    assert torch.equal(sur["factors"], flown[sur["primitive_rows"]])
    assert len(sur["names"]) == 17 and "turbulence" not in " ".join(sur["names"]) and "dead_draw" not in sur["names"]
    assert sur["fit_ok"].all() and sur["n_fit"] + sur["n_val"] == sur["count"] and sur["n_val"] == sur["count"] // 4
    pred = mc_engine_predict(sur)
    summ = run_["summary"].cpu().numpy()
    fac = sur["factors"].cpu().numpy()
    from erpl_monte_carlo_sim_amd import analysis
    why = analysis._filter(run_["summary"], run_.get("status"), None)[2].cpu().numpy()
    ys = summ[sur["rows"]]
    members, fit, val, _, _ = R.population(fac, ys, why, 4)
    assert len(members) == sur["count"]
    for j in range(len(sur["rows"])):
        tss, rss, r2 = R.residuals(ys[j, fit], pred[j, fit])
        close(sur["r2"][j], r2)
        tss, rss, q2 = R.residuals(ys[j, val], pred[j, val])
        close(sur["q2"][j], q2)
        print(f"{sur['row_names'][j]}: r2 {sur['r2'][j]:.4f} q2 {sur['q2'][j]:.4f}; total indices first: {sur['ranking'][j][:3]}")
    assert np.array_equal(sur["validation"]["samples"], val[:4096])
    with pytest.raises(ValueError, match="independent"):
        mc.surrogate({"summary": run_["summary"]})


def mc_engine_predict(sur):
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    return shared_engine(sur["factors"].device).surrogate_predict(sur["model"], sur["factors"]).cpu().numpy()
