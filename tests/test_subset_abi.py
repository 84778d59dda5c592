"""erpl_mc_subset_* at the C boundary, no GPU: the struct mirrors, the defaults, the _host calls against the NumPy restatement
(subset_ref), the whole run on a linear limit state, every refusal in the header's order, the host check program."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import special

import helpers as H
import subset_cases as SC
import subset_ref as R
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
DUMMY = H.DUMMY
ERR_INVALID = -1     # ERPL_ERR_INVALID
NAMES = ("limit_state", "seeds", "propose", "commit", "chain_stats")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


# ------------------------------------------------------------------------------------------------ the boundary
def test_struct_layout_matches_the_c_compiler(tmp_path):
    H.check_struct_layouts(tmp_path, (("erpl_subset_spec", "ErplSubsetSpec"), ("erpl_subset_gather", "ErplSubsetGather"),
                                      ("erpl_subset_triple", "ErplSubsetTriple")),
                           (("ERPL_SUBSET_MAX_STEPS", _abi.SUBSET_MAX_STEPS), ("ERPL_SUBSET_MAX_SLOTS", _abi.SUBSET_MAX_SLOTS)))


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ["erpl_mc_subset_defaults"] + [f"erpl_mc_subset_{n}{h}" for n in NAMES for h in ("", "_host")]:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)
    assert _abi.ABI_VERSION == 4


def test_defaults_are_exact(lib):
    spec = _abi.ErplSubsetSpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_subset_defaults(C.byref(spec)) == 0
    ana = _abi.ErplAnalysisSpec()
    assert lib.erpl_mc_analysis_defaults(C.byref(ana)) == 0
    for name in ("max_apogee", "min_apogee", "max_range", "max_flight_time", "energy_apogee"):
        assert getattr(spec, name) == getattr(ana, name)
    assert (spec.row, spec.sign, spec.use_centre, spec.reserved, spec.cx, spec.cy) == (_abi.SUM_RANGE, 1, 0, 0, 0.0, 0.0)
    assert (spec.seed, spec.level, spec.step) == (0, 0, 1)
    assert lib.erpl_mc_subset_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


# ------------------------------------------------------------------------------------------------ 1. proposals
def host_propose(step, level, cur, first_chain=0, rho=SC.PROPOSE_RHO, w=SC.PROPOSE_W, ld_out=None):
    count = cur.shape[1]
    out = np.full((5, ld_out or count + 3), -7.0)
    spec = analysis.subset_spec(seed=SC.PROPOSE_SEED, level=level, step=step)
    analysis.subset_propose_host(spec, SC.PROPOSE_KINDS, rho, cur, first_chain, out[:, :count], w=w)
    assert np.all(out[:, count:] == -7.0)      # nothing behind count
    return out[:, :count]


@pytest.mark.parametrize("step,level", SC.PROPOSE_POINTS)
def test_proposals_match_the_restatement(lib, step, level):
    cur = SC.propose_current()[:, :SC.PROPOSE_CHAINS]      # a view: ld = 137 > count = 130
    got = host_propose(step, level, cur)
    SC.check_proposal(got, cur, step, level)
    first, count = SC.WINDOW
    win = host_propose(step, level, cur[:, first:first + count], first_chain=first)
    assert np.array_equal(win.view(np.uint64), got[:, first:first + count].view(np.uint64))


def test_proposals_wrap_at_both_ends_and_honour_rho_0_and_1(lib):
    cur = SC.propose_current()[:, :SC.PROPOSE_CHAINS]
    got = host_propose(1, 0, cur)
    want = SC.check_proposal(got, cur, 1, 0)
    u = R.uniforms(SC.PROPOSE_SEED, 0, 1, 5, 0, SC.PROPOSE_CHAINS)
    raw = cur[4] + 1.0 * (u[4] - 0.5)
    assert np.any(raw < 0.0) and np.any(raw >= 1.0)                 # both wraps happen in the row of width 1
    assert np.array_equal(got[4], want[4])
    fresh = host_propose(1, 0, cur, rho=np.zeros(5))
    copy = host_propose(1, 0, cur, rho=np.ones(5), w=np.zeros(5))
    xi = special.ndtri(u[:3])
    assert np.all(np.abs(fresh[:3] - xi) <= 8e-15 * np.maximum(1.0, np.abs(xi)))
    assert np.array_equal(copy[:3], cur[:3])
    assert np.array_equal(copy[3:, 8:], cur[3:, 8:])                  # width 0: a copy (the first columns hold the clamps' inputs)


# ------------------------------------------------------------------------------------------------ 2. seed selection
@pytest.mark.parametrize("name,g,n_seeds", SC.seed_cases(), ids=[c[0] for c in SC.seed_cases()])
def test_seed_selection_is_a_lexsort(lib, name, g, n_seeds):
    n = g.size
    src = np.arange(3 * n, dtype=np.float64).reshape(3, n)
    dst = np.full((3, n_seeds + 2), -1.0)
    st_src, st_dst = np.arange(n, dtype=np.int32) * 3, np.full(n_seeds, -1, dtype=np.int32)
    idx, sel, thr, alive = analysis.subset_seeds_host(g, n_seeds, [(src, dst[:, :n_seeds]), (st_src, st_dst)])
    SC.check_seeds(g, n_seeds, idx, sel, thr, alive)
    assert np.array_equal(dst[:, :n_seeds], src[:, idx]) and np.all(dst[:, n_seeds:] == -1.0) and np.array_equal(st_dst, st_src[idx])
    _, ind, _, count = analysis.subset_seeds_host(g, 0, threshold=thr)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(ind, (g >= thr).astype(np.uint8)) and count == int(ind.sum())


def test_a_died_out_level_is_refused(lib):
    g = np.array([1.0, -np.inf, np.nan, 2.0, -np.inf])
    idx, sel, thr, alive = analysis.subset_seeds_host(g, 2)
    assert list(idx) == [0, 3] and thr == 1.0 and alive == 2
    with pytest.raises(_abi.ErplError, match="died out"):
        analysis.subset_seeds_host(g, 3)


# ------------------------------------------------------------------------------------------------ 3. chain statistics, commit
@pytest.mark.parametrize("name,sel,chains,steps", SC.chain_cases(), ids=[c[0] for c in SC.chain_cases()])
def test_chain_statistics_match_the_double_loop(lib, name, sel, chains, steps):
    n1, pair = analysis.subset_chain_stats_host(sel, chains, steps)
    w_n1, w_pair = R.chain_stats(sel, chains, steps)
    assert n1 == w_n1 and np.array_equal(pair, w_pair)
    if 0 < n1 < chains * steps:
        p, delta, gamma = analysis.subset_delta(n1, pair, chains, steps, True)
        assert np.allclose((p, delta, gamma), R.delta(n1, w_pair, chains, steps, True), rtol=1e-13, atol=1e-15)


def test_commit_takes_the_candidate_iff_it_reaches_the_threshold(lib):
    rng = np.random.default_rng(2)
    count = 130
    g_cur, g_cand = rng.normal(size=count), rng.normal(size=count)
    g_cand[:4] = [0.25, np.nextafter(0.25, 0.0), np.nan, np.inf]
    cand, cur = rng.normal(size=(5, count)), rng.normal(size=(5, 2 * count))
    st_cand, st = rng.integers(0, 9, count).astype(np.int32), rng.integers(0, 9, 2 * count).astype(np.int32)
    g_both = np.concatenate([g_cur, np.full(count, -9.0)])
    acc = analysis.subset_commit_host(0.25, g_cand, g_both[:count], g_both[count:],
                                      [(cand, cur[:, :count], cur[:, count:]), (st_cand, st[:count], st[count:])])
    take = g_cand >= 0.25
    assert take[0] and not take[1] and not take[2] and take[3] and acc == int(take.sum())
    assert np.array_equal(g_both[count:], np.where(take, g_cand, g_cur))
    assert np.array_equal(cur[:, count:], np.where(take, cand, cur[:, :count]))
    assert np.array_equal(st[count:], np.where(take, st_cand, st[:count]))


def test_limit_state_matches_the_restatement(lib):
    summ, status = SC.limit_state_inputs()
    for name, spec, kw in SC.limit_state_specs():
        kw = dict(kw)
        want = R.limit_state(summ, status, kw.pop("bounds", SC.BOUNDS), **kw)
        got = analysis.subset_limit_state_host(spec, summ, status)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
        if name == "range-upper":
            assert list(np.flatnonzero(np.isneginf(got[:16]))) == [3, 4, 5, 6, 7, 8, 10, 11] and np.isfinite(got[9])
        if name == "row15-upper":
            assert np.isneginf(got[12])
        if name == "miss":
            assert np.isneginf(got[13])
    no_status = analysis.subset_limit_state_host(SC.limit_state_specs()[0][1], summ, None)
    assert np.isfinite(no_status[10]) and np.isfinite(no_status[11])


# ------------------------------------------------------------------------------------------------ 4. the whole run
linear_draws0 = SC.linear_draws0


@pytest.mark.parametrize("target,exact,sized_cov,seed", SC.LINEAR_TARGETS)
def test_linear_limit_state_through_the_host_calls(lib, target, exact, sized_cov, seed):
    """Measured at the committed seeds (restatement and host calls alike): target 4.7534, seed 11: P = 1.368e-6,
    cov = 0.183, |ln(P / exact)| / cov = 1.71; target 3.0902, seed 12: P = 1.0142e-3, cov = 0.104, ratio = 0.13."""
    chains, steps = SC.LINEAR_CHAINS, SC.LINEAR_STEPS
    ref = R.run(SC.linear_g, linear_draws0(seed), SC.LINEAR_KINDS, chains, steps, target, rho=SC.LINEAR_RHO, seed=seed)
    SC.check_linear(ref, exact, sized_cov)                       # the restatement alone meets the condition
    out = analysis.subset_simulation(SC.linear_g, linear_draws0(seed), SC.LINEAR_KINDS, chains=chains, steps=steps, target=target,
                                     rho=SC.LINEAR_RHO, seed=seed)
    ratio = SC.check_linear(out, exact, sized_cov)
    print(f"target {target}: P = {out['probability']:.6g}, cov = {out['cov']:.4f}, ratio = {ratio:.3f}")
    levels = len(out["levels"])
    assert out["reached"] and [lv["n1"] for lv in out["levels"]] == ref["n1"] and all(n1 == chains for n1 in ref["n1"][:-1])
    assert levels == (7 if target > 4 else 4)
    N = chains * steps
    assert out["samples"] == levels * N and out["evaluations"] == N + (levels - 1) * (steps - 1) * chains == ref["evaluations"]
    assert np.allclose(out["thresholds"], ref["thresholds"], rtol=1e-12, atol=0)
    assert math.isclose(out["probability"], ref["probability"], rel_tol=1e-12) and math.isclose(out["cov"], ref["cov"], rel_tol=1e-9)
    assert out["interval"][0] < out["probability"] < out["interval"][1]
    curve = out["curve"]
    assert np.all(np.diff(curve[:, 0]) >= 0) and np.all(np.diff(curve[:, 1]) <= 0) and curve[0, 1] == 1.0
    pop = out["population"]
    assert np.all(pop["g"] >= out["thresholds"][-2]) and np.array_equal(pop["indicator"], (pop["g"] >= target).astype(np.uint8))
    again = analysis.subset_simulation(SC.linear_g, linear_draws0(seed), SC.LINEAR_KINDS, chains=chains, steps=steps, target=target,
                                       rho=SC.LINEAR_RHO, seed=seed)
    assert again["probability"] == out["probability"] and np.array_equal(again["population"]["draws"], pop["draws"])


def test_driver_refusals_and_the_curve_without_a_target(lib):
    x = linear_draws0(3)[:, :64 * 4]
    out = analysis.subset_simulation(SC.linear_g, x, SC.LINEAR_KINDS, chains=64, steps=4, max_levels=2, seed=3)
    assert len(out["levels"]) == 2 and out["probability"] == 0.25 ** 2 and not out["reached"]
    assert out["thresholds"][1] > out["thresholds"][0] and np.all(out["population"]["g"] >= out["thresholds"][1])
    assert np.all(out["population"]["indicator"] == 1) and out["evaluations"] == 256 + 2 * 3 * 64
    dead = lambda d: np.where(np.arange(d.shape[1]) < 10, SC.linear_g(d), -np.inf)
    with pytest.raises(ValueError, match="fewer than chains"):
        analysis.subset_simulation(dead, x, SC.LINEAR_KINDS, chains=64, steps=4)
    with pytest.raises(ValueError):
        analysis.subset_simulation(SC.linear_g, x, SC.LINEAR_KINDS, chains=64, steps=5)


def test_chains_that_do_not_move_are_reported(lib):
    """An evaluator whose candidates never reach the threshold: the levels slice the frozen level-0 sample, and the result says so."""
    x = linear_draws0(3)[:, :256]
    calls = [0]

    def frozen(d):
        calls[0] += 1
        return SC.linear_g(d) if calls[0] == 1 else np.full(d.shape[1], -np.inf)
    out = analysis.subset_simulation(frozen, x, SC.LINEAR_KINDS, chains=64, steps=4, max_levels=2, seed=3)
    assert [lv["acceptance"] for lv in out["levels"]] == [0.0, 0.0] and out["levels"][1]["gamma"] == pytest.approx(3.0)
    assert len(out["warnings"]) == 2 and all("do not move" in w for w in out["warnings"])
    healthy = analysis.subset_simulation(SC.linear_g, x, SC.LINEAR_KINDS, chains=64, steps=4, max_levels=2, seed=3)
    assert healthy["warnings"] == []


# ------------------------------------------------------------------------------------------------ 5. every refusal
def refusals():
    """(entry, keyword overrides, a word of the message), in the order of the header."""
    bad_spec = lambda **kw: {"spec_fields": kw}
    out = [("limit_state", {"spec": None}, "spec"), ("limit_state", {"summary": None}, "summary"), ("limit_state", {"g": None}, "g is"),
           ("limit_state", bad_spec(max_range=math.nan), "bound"), ("limit_state", bad_spec(row=16), "row"),
           ("limit_state", bad_spec(sign=0), "sign"), ("limit_state", bad_spec(use_centre=1, cx=math.inf), "centre"),
           ("limit_state", {"n": 0}, "n ="), ("limit_state", {"n": 2 ** 31}, "n ="), ("limit_state", {"ld": 7}, "ld"),
           ("limit_state", {"ctx": None}, "ctx")]
    out += [("seeds", {"g": None}, "g is"), ("seeds", {"selected": None}, "selected"), ("seeds", {"threshold": None}, "threshold"),
            ("seeds", {"n_alive": None}, "n_alive"), ("seeds", {"n": 0}, "n ="), ("seeds", {"n_seeds": -1}, "n_seeds"),
            ("seeds", {"n_seeds": 9}, "n_seeds"), ("seeds", {"idx": None}, "idx"), ("seeds", {"n_slots": 5}, "n_gathers"),
            ("seeds", {"n_slots": 1, "n_seeds": 0}, "n_gathers"), ("seeds", {"slots": None}, "gathers is"),
            ("seeds", {"slot": {"src": None}}, "src"), ("seeds", {"slot": {"dst": None}}, "dst"), ("seeds", {"slot": {"rows": 0}}, "rows"),
            ("seeds", {"slot": {"rows": 4097}}, "rows"), ("seeds", {"slot": {"elem_size": 2}}, "elem_size"),
            ("seeds", {"slot": {"ld_src": 7}}, "ld_src"), ("seeds", {"slot": {"ld_dst": 3}}, "ld_dst"), ("seeds", {"ctx": None}, "ctx")]
    out += [("propose", {"spec": None}, "spec")] + [("propose", {k: None}, f"{k} is") for k in ("kinds", "rho", "s", "w", "cur", "cand")]
    out += [("propose", {"rows": 0}, "rows"), ("propose", {"rows": 4097}, "rows"), ("propose", bad_spec(step=65536), "step"),
            ("propose", {"first_chain": -1}, "first_chain"), ("propose", {"n": -1}, "count"),
            ("propose", {"first_chain": 2 ** 31 - 4}, "first_chain + count"), ("propose", {"ld": 7}, "ld ="), ("propose", {"ld_cand": 7}, "ld_cand"),
            ("propose", {"kinds": bytes([1, 2])}, "kinds[1]"), ("propose", {"rho": [0.5, 1.5]}, "rho[1]"), ("propose", {"rho": [math.nan, 0.5]}, "rho[0]"),
            ("propose", {"s": [-0.1, 0.5]}, "s[0]"), ("propose", {"w": [0.5, 2.0]}, "w[1]"), ("propose", {"ctx": None}, "ctx")]
    out += [("commit", {k: None}, f"{k} is") for k in ("threshold", "g_cand", "g_cur", "g_next", "n_accepted")]
    out += [("commit", {"n_slots": -1}, "n_triples"), ("commit", {"n_slots": 5}, "n_triples"), ("commit", {"slots": None}, "triples is"),
            ("commit", {"slot": {"cand": None}}, "cand"), ("commit", {"slot": {"cur": None}}, "cur"), ("commit", {"slot": {"next": None}}, "next"),
            ("commit", {"slot": {"rows": 0}}, "rows"), ("commit", {"slot": {"elem_size": 3}}, "elem_size"),
            ("commit", {"slot": {"ld_cand": 7}}, "ld_cand"), ("commit", {"slot": {"ld": 7}}, ".ld ="), ("commit", {"n": -1, "n_slots": 0}, "count"),
            ("commit", {"ctx": None}, "ctx")]
    out += [("chain_stats", {"selected": None}, "selected"), ("chain_stats", {"n1": None}, "n1"), ("chain_stats", {"chains": 0}, "chains"),
            ("chain_stats", {"steps": 0}, "steps"), ("chain_stats", {"steps": 65536}, "steps"),
            ("chain_stats", {"chains": 2 ** 31 // 4, "steps": 4}, "chains * steps"), ("chain_stats", {"pair": None}, "pair"),
            ("chain_stats", {"ctx": None}, "ctx")]
    return out


def call_entry(lib, entry, host, kw):
    """One call with good arguments (host pointers that are never dereferenced: every refusal comes first) but for `kw`."""
    kw = dict(kw)
    ctx = kw.pop("ctx", DUMMY)
    spec = _abi.ErplSubsetSpec()
    assert lib.erpl_mc_subset_defaults(C.byref(spec)) == 0
    for k, v in kw.pop("spec_fields", {}).items():
        setattr(spec, k, v)
    sp = None if "spec" in kw and kw.pop("spec") is None else C.byref(spec)
    arg = lambda k: kw.pop(k) if k in kw else DUMMY
    n = kw.pop("n", 8)
    n_slots = kw.pop("n_slots", 1)
    if entry == "seeds":
        slot = _abi.ErplSubsetGather(0x1000, 0x1000, 8, 4, 2, 8)
    else:
        slot = _abi.ErplSubsetTriple(0x1000, 0x1000, 0x1000, 8, 8, 2, 8)
    for k, v in kw.pop("slot", {}).items():
        setattr(slot, k, v)
    slots = (type(slot) * 1)(slot)
    slots = None if "slots" in kw and kw.pop("slots") is None else slots
    fn = getattr(lib, f"erpl_mc_subset_{entry}" + ("_host" if host else ""))
    head, tail = ([] if host else [ctx]), ([] if host else [None])
    if entry == "limit_state":
        args = [sp, arg("summary"), None, kw.pop("ld", 8), n, arg("g")]
    elif entry == "seeds":
        args = [arg("g"), n, kw.pop("n_seeds", 4), arg("idx"), arg("selected"), arg("threshold"), arg("n_alive"), slots, n_slots]
    elif entry == "propose":
        rows = kw.pop("rows", 2)
        vec = lambda k: None if k in kw and kw[k] is None else (C.c_double * 2)(*kw.get(k, [0.5, 0.5]))
        rho, s, w = vec("rho"), vec("s"), vec("w")
        for k in ("rho", "s", "w"):
            kw.pop(k, None)
        kinds = kw.pop("kinds") if "kinds" in kw else bytes([1, 0])
        args = [sp, kinds, rho, s, w, rows, arg("cur"), kw.pop("ld", 8), kw.pop("first_chain", 0), n, arg("cand"), kw.pop("ld_cand", 8)]
    elif entry == "commit":
        args = [arg("threshold"), arg("g_cand"), arg("g_cur"), arg("g_next"), slots, n_slots, n, arg("n_accepted")]
    else:
        args = [arg("selected"), kw.pop("chains", 4), kw.pop("steps", 2), arg("n1"), arg("pair")]
    assert not kw, kw
    return fn(*(head + args + tail))


@pytest.mark.parametrize("entry,kw,word", refusals(), ids=[f"{e}-{i}" for i, (e, _, _) in enumerate(refusals())])
def test_every_refusal_names_its_argument(lib, entry, kw, word):
    for host in (False, True):
        if "ctx" in kw and host:
            continue
        assert call_entry(lib, entry, host, kw) == ERR_INVALID, (entry, kw, host)
        assert word.encode() in lib.erpl_mc_last_error(), (entry, kw, lib.erpl_mc_last_error())


def test_refusals_come_in_the_order_of_the_header(lib):
    """Two faults at once: the one the header lists first is reported."""
    assert call_entry(lib, "limit_state", True, {"summary": None, "n": 0}) == ERR_INVALID and b"summary" in lib.erpl_mc_last_error()
    assert call_entry(lib, "seeds", True, {"n": 0, "n_seeds": -1}) == ERR_INVALID and b"n =" in lib.erpl_mc_last_error()
    assert call_entry(lib, "propose", True, {"rows": 0, "ld": 7}) == ERR_INVALID and b"rows" in lib.erpl_mc_last_error()
    assert call_entry(lib, "propose", True, {"ld": 7, "rho": [2.0, 0.5]}) == ERR_INVALID and b"ld =" in lib.erpl_mc_last_error()
    assert call_entry(lib, "commit", True, {"g_next": None, "n_slots": 9}) == ERR_INVALID and b"g_next" in lib.erpl_mc_last_error()
    assert call_entry(lib, "chain_stats", False, {"steps": 0, "ctx": None}) == ERR_INVALID and b"steps" in lib.erpl_mc_last_error()


# ------------------------------------------------------------------------------------------------ 6. the host check program
def test_the_host_check_program_passes(lib):
    exe = os.path.join(CSRC, "erpl_subset_check")
    assert os.path.exists(exe), "erpl_subset_check is built by `make all` (build())"
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("ok erpl_subset_check") and "FAIL" not in res.stdout
