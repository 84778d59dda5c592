"""erpl_mc_design, its defaults and erpl_mc_design_host at the C boundary, as far as it goes without a GPU: the tests' own
restatement of the contract (design_ref) against the contract's known answers, struct layout against gcc, the defaults, every
refusal (before any device work, in the order the header lists, the context last: a NULL context and dummy pointers show
them all), the host copy of the design against design_ref bit for bit and against scipy's normal quantile, and what makes
a design worth flying: strata, Kolmogorov distance, rank correlations, variance of a near-additive mean."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import special

import helpers as H
from erpl_monte_carlo_sim_amd import _abi

import design_cases as DC
import design_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
DUMMY = H.DUMMY
U, N = _abi.DESIGN_UNIFORM, _abi.DESIGN_NORMAL
KINDS = (_abi.DESIGN_RANDOM, _abi.DESIGN_LHS, _abi.DESIGN_LHS_CENTRED)


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_design_ref_reproduces_the_known_answers_of_the_contract():
    keys = {(1234, 3): "a05e3810 979fc8eb 64b88d40 2885b1cb 3566db8c fb37ac5a",
            (0, 0): "dd2fc514 adf5a0db e6f70b22 d3b4ca74 bc42f20e ac0ddcde"}
    for (seed, row), want in keys.items():
        assert " ".join("%08x" % k for k in R.round_keys(seed, row)) == want
    perms = ((1234, 3, 5, [3, 0, 2, 4, 1]), (1234, 3, 17, [14, 11, 8, 3, 16, 1, 10, 0]),
             (1234, 3, 1000, [888, 992, 520, 846, 557, 197, 817, 804]), (0, 0, 7, [5, 2, 0, 3, 6, 1, 4]),
             (2 ** 40 + 5, 318, 100000, [79270, 90820, 43353, 74263, 40972, 35430, 26576, 54572]))
    for seed, row, m, want in perms:
        assert R.perm(R.round_keys(seed, row), m, np.arange(min(m, 8))).tolist() == want, (seed, row, m)
    jit = {(1234, 3): ["0x1.b3872a6a6699ap-1", "0x1.afb89b4a9f2f2p-1", "0x1.6c330931e29d7p-2"],
           (0, 0): ["0x1.348e23f2dce74p-4", "0x1.450f55b7f9f1cp-1", "0x1.44311527a54d7p-2"]}
    for (seed, row), want in jit.items():
        assert [float(u).hex() for u in R.jitter(seed, row, [0, 1, 2])] == want
    assert [R.half_bits(m) for m in (1, 4, 5, 16, 17, 64, 65, 2 ** 31 - 1)] == [1, 1, 2, 2, 3, 3, 4, 16]


def test_struct_layout_matches_the_c_compiler(tmp_path):
    H.check_struct_layouts(tmp_path, (("erpl_design_spec", "ErplDesignSpec"),),
                           (("ERPL_DESIGN_MAX_ROWS", _abi.DESIGN_MAX_ROWS), ("ERPL_DESIGN_RANDOM", _abi.DESIGN_RANDOM),
                            ("ERPL_DESIGN_LHS", _abi.DESIGN_LHS), ("ERPL_DESIGN_LHS_CENTRED", _abi.DESIGN_LHS_CENTRED),
                            ("ERPL_DESIGN_UNIFORM", _abi.DESIGN_UNIFORM), ("ERPL_DESIGN_NORMAL", _abi.DESIGN_NORMAL),
                            ("ERPL_ERR_INTERNAL", _abi.ERR_INTERNAL)))
    assert _abi.DESIGN_MAX_ROWS == 4096 and C.sizeof(_abi.ErplDesignSpec) == 40


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("erpl_mc_design_defaults", "erpl_mc_design", "erpl_mc_design_host"):
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def test_defaults_are_exact(lib):
    spec = _abi.ErplDesignSpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_design_defaults(C.byref(spec)) == 0
    assert (spec.kind, spec.rows, spec.first_row, spec.reserved) == (_abi.DESIGN_LHS, 1, 0, 0)
    assert (spec.n, spec.block, spec.seed) == (1, 0, 0)
    assert lib.erpl_mc_design_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


@pytest.mark.parametrize("entry", ["device", "host"])
def test_refusals_come_before_any_device_work_in_the_documented_order(lib, entry):
    good_kinds = bytes([N, U, N, U])

    def call(spec, kinds=good_kinds, first=0, count=8, out=DUMMY, ld=8):
        sp = C.byref(spec) if spec is not None else None
        if entry == "device":
            rc = lib.erpl_mc_design(None, sp, kinds, first, count, out, ld, None)
        else:
            rc = lib.erpl_mc_design_host(sp, kinds, first, count, out, ld)
        return rc, lib.erpl_mc_last_error().decode()

    def broken(**fields):
        """A spec and a call with EVERY later check failing too: the earlier one has to be the one reported."""
        spec = DC.spec_of(7, 0, 0, -1, -1)
        for k, v in fields.items():
            setattr(spec, k, v)
        return spec

    bad_kinds = bytes([N, 2, N, U])
    late = dict(kinds=bad_kinds, first=-1, count=-1, ld=-2)
    # 1. NULL spec, kinds, out
    rc, msg = call(None, kinds=None, out=None)
    assert rc == -1 and "spec" in msg
    rc, msg = call(broken(), kinds=None, out=None)
    assert rc == -1 and "kinds" in msg
    rc, msg = call(broken(), **dict(late, out=None))
    assert rc == -1 and "out" in msg
    # 2. kind
    for bad in (3, -1, 7):
        rc, msg = call(broken(kind=bad), **late)
        assert rc == -1 and "kind" in msg and str(bad) in msg
    # 3. rows / first_row
    for rows, first_row in ((0, 0), (-1, 0), (1, -1), (4097, 0), (1, 4096), (2, 4095)):
        rc, msg = call(broken(kind=1, rows=rows, first_row=first_row), **late)
        assert rc == -1 and "rows" in msg and "first_row" in msg and str(rows) in msg
    # 4. n
    for n in (0, -5, 2 ** 31, 2 ** 40):
        rc, msg = call(broken(kind=1, rows=4, first_row=0, n=n), **late)
        assert rc == -1 and f"n = {n}" in msg
    # 5. block
    for block in (-1, 13, 5, 24):
        rc, msg = call(broken(kind=1, rows=4, first_row=0, n=12, block=block), **late)
        assert rc == -1 and f"block = {block}" in msg
    ok = DC.spec_of(_abi.DESIGN_LHS, 4, 12, 4)
    # 6. first, count, first + count
    rc, msg = call(ok, **dict(late, count=1))
    assert rc == -1 and "first" in msg
    rc, msg = call(ok, **dict(late, first=0))
    assert rc == -1 and "count" in msg
    for first, count in ((0, 13), (12, 1), (13, 0), (5, 8)):
        rc, msg = call(ok, kinds=bad_kinds, first=first, count=count, ld=-2)
        assert rc == -1 and "first + count" in msg
    # 7. ld
    rc, msg = call(ok, kinds=bad_kinds, first=2, count=10, ld=9)
    assert rc == -1 and "ld" in msg
    # 8. kinds
    rc, msg = call(ok, kinds=bad_kinds, first=2, count=10, ld=10)
    assert rc == -1 and "kinds[1]" in msg
    if entry == "host":
        return
    # 9. everything in order, at the limits: only the context is left
    rc, msg = call(ok, first=2, count=10, ld=10)
    assert rc == -1 and "ctx" in msg
    rc, msg = call(ok, first=12, count=0, ld=0)
    assert rc == -1 and "ctx" in msg
    big = DC.spec_of(_abi.DESIGN_LHS_CENTRED, 4096, 2 ** 31 - 1, 1, 0, 2 ** 64 - 1)
    rc, msg = call(big, kinds=bytes(4096), first=0, count=2 ** 31 - 1, ld=2 ** 31 - 1)
    assert rc == -1 and "ctx" in msg
    rc, msg = call(DC.spec_of(_abi.DESIGN_RANDOM, 1, 1, 1, 4095), kinds=bytes([N]), count=1, ld=1)
    assert rc == -1 and "ctx" in msg


def test_count_zero_is_ok_and_writes_nothing(lib):
    out = DC.host_design(lib, _abi.DESIGN_LHS, [N, U], 12, first=12, count=0, pad=3, fill=-7.0)
    assert out.shape == (2, 3) and np.all(out == -7.0)


def test_the_header_alone_on_the_host():
    """csrc/erpl_design_check: erpl_design.h without the library - every stratum of every replicate of every shape once,
    windows equal to the full rows.  (The same program is what a host sanitizer build runs.)"""
    subprocess.run(["make", "-s", "-C", CSRC, "erpl_design_check"], check=True)     # (nothing to do after build())
    r = subprocess.run([os.path.join(CSRC, "erpl_design_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") >= len(DC.SHAPES)


@pytest.mark.parametrize("shape", DC.SHAPES, ids=DC.shape_id)
def test_host_design_equals_the_reference(lib, shape):
    """Uniform rows bit for bit in all three kinds, normal rows against ndtri of the reference's p; ld = count + 3 with a
    sentinel behind every row; the window equals those columns of the full call; two calls return the same bytes."""
    rows, n, block, first, count, first_row = shape
    for kind in KINDS:
        p_ref, _ = R.design(DC.SEED, kind, rows, n, block, first, count, first_row)
        assert np.all((p_ref > 0.0) & (p_ref < 1.0))
        got = DC.host_design(lib, kind, [U] * rows, n, block, first, count, first_row, pad=3, fill=-7.0)
        assert np.array_equal(got[:, :count], p_ref) and np.all(got[:, count:] == -7.0), kind
        again = DC.host_design(lib, kind, [U] * rows, n, block, first, count, first_row, pad=3, fill=-7.0)
        assert got.tobytes() == again.tobytes()
        mixed = [N if r % 2 == 0 else U for r in range(rows)]
        got = DC.host_design(lib, kind, mixed, n, block, first, count, first_row)
        assert np.array_equal(got[1::2], p_ref[1::2])
        DC.assert_normals(got[0::2], p_ref[0::2])
        if n <= 70000:
            full = DC.host_design(lib, kind, mixed, n, block, 0, n, first_row)
            assert np.array_equal(full[:, first:first + count], got)


@pytest.mark.parametrize("shape", DC.SHAPES, ids=DC.shape_id)
def test_every_replicate_hits_every_stratum_once(lib, shape):
    """The rank of a value within its replicate is the reference's pi, so every row of every replicate is a permutation of
    its m strata; LHS_CENTRED is exactly (pi + 0.5) / m."""
    rows, n, block, _, _, first_row = shape
    m = block or n
    _, pi = R.design(DC.SEED, _abi.DESIGN_LHS, rows, n, block, 0, n, first_row)
    assert np.array_equal(np.sort(pi.reshape(rows, n // m, m), axis=2), np.broadcast_to(np.arange(m), (rows, n // m, m)))
    p = DC.host_design(lib, _abi.DESIGN_LHS, [U] * rows, n, block, first_row=first_row)
    assert np.array_equal(DC.ranks_in_replicates(p, m), pi)
    assert np.array_equal(np.floor(p * m).astype(np.int64), pi)     # no p of these shapes sits within an ulp of an edge
    z = DC.host_design(lib, _abi.DESIGN_LHS, [N] * rows, n, block, first_row=first_row)
    assert np.array_equal(DC.ranks_in_replicates(z, m), pi)
    c = DC.host_design(lib, _abi.DESIGN_LHS_CENTRED, [U] * rows, n, block, first_row=first_row)
    assert np.array_equal(c, (pi + 0.5) / m)


def test_replicates_of_one_row_are_different_permutations(lib):
    p = DC.host_design(lib, _abi.DESIGN_LHS, [U] * 6, 4096, 512)
    pi = DC.ranks_in_replicates(p, 512).reshape(6, 8, 512)
    for r in range(6):
        for a in range(8):
            for b in range(a + 1, 8):
                assert not np.array_equal(pi[r, a], pi[r, b]), (r, a, b)
    for r in range(5):      # and those of different rows
        assert not np.array_equal(pi[r], pi[r + 1])


def test_kolmogorov_distance_of_a_normal_lhs_row(lib):
    """By construction: the k-th smallest p lies in [k / n, (k + 1) / n), so the empirical distribution of z is within 1 / n
    of the normal one."""
    n = 4096
    z = np.sort(DC.host_design(lib, _abi.DESIGN_LHS, [N], n)[0])
    cdf = special.ndtr(z)
    k = np.arange(n)
    d = max(np.max((k + 1) / n - cdf), np.max(cdf - k / n))
    assert d <= 1.0 / n + 1e-12, d


def _spearman_matrix(x):
    return np.corrcoef(np.argsort(np.argsort(x, axis=1), axis=1).astype(np.float64))


@pytest.mark.parametrize("n", [4096, 5000, 257])
def test_rows_are_uncorrelated_with_each_other_with_the_column_index_and_with_themselves(lib, n):
    """|Spearman| <= 5 / sqrt(n): over the 2016 pairs of 64 rows (independent permutations exceed 5 about once in a thousand
    such runs), of every row with the column index, and of every row with itself shifted by one column."""
    p = DC.host_design(lib, _abi.DESIGN_LHS, [U] * 64, n)
    rho = _spearman_matrix(p)
    worst = np.abs(rho - np.eye(64)).max()
    print(f"n={n}: max |rho| sqrt(n) = {worst * np.sqrt(n):.3f}")
    assert worst <= 5.0 / np.sqrt(n)
    with_index = np.abs(_spearman_matrix(np.vstack([p, np.arange(n, dtype=np.float64)]))[64, :64]).max()
    lag = max(abs(_spearman_matrix(np.vstack([p[r, :-1], p[r, 1:]]))[0, 1]) for r in range(64))
    print(f"n={n}: index {with_index * np.sqrt(n):.3f}, lag one {lag * np.sqrt(n):.3f}")
    assert with_index <= 5.0 / np.sqrt(n) and lag <= 5.0 / np.sqrt(n)


def test_lhs_cuts_the_variance_of_a_near_additive_mean(lib):
    """The mean of sum c_r z_r + 0.3 z_0^2 + 0.5 z_1 z_2 over n = 256, seeds 0..199: LHS at most 0.05 of RANDOM's variance
    (0.0068 in the contract's prototype; the bound leaves a factor 7 for the noise of 200 seeds)."""
    est = {kind: [DC.additive_estimator(DC.host_design(lib, kind, [N] * 20, 256, seed=s)) for s in range(200)]
           for kind in (_abi.DESIGN_RANDOM, _abi.DESIGN_LHS)}
    ratio = np.var(est[_abi.DESIGN_LHS]) / np.var(est[_abi.DESIGN_RANDOM])
    print(f"variance ratio LHS / RANDOM = {ratio:.5f}")
    assert ratio <= 0.05
    assert abs(np.mean(est[_abi.DESIGN_LHS]) - 0.3) < 0.01      # E = 0.3 E z^2


def test_engine_design_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.design: the refusal is on the host, before the library is called."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    eng.lib = H.load_lib()
    with pytest.raises(ValueError, match="out"):
        TrajectoryEngine.design(eng, [N, U], 8, 0, out=torch.zeros((2, 8), dtype=torch.float64))
