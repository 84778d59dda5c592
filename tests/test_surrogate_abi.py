"""erpl_mc_surrogate and its companions at the C boundary, as far as it goes without a GPU: struct layout against gcc, the
defaults, symbols declared / exported / documented, every refusal (before any device work, in the order the header lists, the
context last: a NULL context and dummy pointers show them all), the terms against the tests' own restatement (surrogate_ref)
and the closed form, erpl_pce.h alone on the host (also under a host sanitizer, as a stand-alone program),
erpl_mc_surrogate_predict_host against surrogate_ref bit for bit, and the reference itself against the analytic Sobol indices
of Ishigami's function."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi

import surrogate_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
DUMMY = H.DUMMY
U, N = _abi.DESIGN_UNIFORM, _abi.DESIGN_NORMAL
SHAPES = {(1, 1, 1): 2, (1, 12, 1): 13, (2, 12, 2): 91, (3, 12, 3): 455, (4, 8, 4): 495, (6, 6, 4): 887, (25, 3, 2): 976,
          (32, 2, 2): 561, (32, 12, 1): 385}
NAMES = ("erpl_mc_surrogate_defaults", "erpl_mc_surrogate_terms", "erpl_mc_surrogate", "erpl_mc_surrogate_predict",
         "erpl_mc_surrogate_predict_host")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def spec_of(n_vars=3, n_rows=2, rows=(0, 16), degree=2, order=2, holdout=0):
    s = _abi.ErplSurSpec()
    s.n_vars, s.n_rows, s.degree, s.order, s.holdout = n_vars, n_rows, degree, order, holdout
    for j, r in enumerate(rows):
        s.rows[j] = r
    return s


def lib_terms(lib, n_vars, degree, order):
    P = C.c_int32(-1)
    rc = lib.erpl_mc_surrogate_terms(n_vars, degree, order, C.byref(P), None)
    assert rc == 0, lib.erpl_mc_last_error()
    tm = np.full((P.value, 4, 2), 99, dtype=np.int8)
    assert lib.erpl_mc_surrogate_terms(n_vars, degree, order, C.byref(P), C.c_void_p(tm.ctypes.data)) == 0
    return tm


def host_predict(lib, kinds, degree, order, coef, X, n=None):
    coef = np.ascontiguousarray(np.atleast_2d(coef), dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    ld = X.shape[1]
    out = np.full((coef.shape[0], ld), -7.0)
    s = spec_of(len(kinds), coef.shape[0], (), degree, order)
    rc = lib.erpl_mc_surrogate_predict_host(C.byref(s), bytes(kinds), C.c_void_p(coef.ctypes.data), C.c_void_p(X.ctypes.data), ld,
                                            ld if n is None else n, C.c_void_p(out.ctypes.data))
    assert rc == 0, lib.erpl_mc_last_error()
    return out


def test_struct_layout_matches_the_c_compiler(tmp_path):
    H.check_struct_layouts(tmp_path, (("erpl_sur_spec", "ErplSurSpec"), ("erpl_sur_row", "ErplSurRow"), ("erpl_surrogate", "ErplSurrogate")),
                           (("ERPL_SUR_MAX_VARS", _abi.SUR_MAX_VARS), ("ERPL_SUR_MAX_ROWS", _abi.SUR_MAX_ROWS),
                            ("ERPL_SUR_ROW_EXTRA", _abi.SUR_ROW_EXTRA), ("ERPL_SUR_MAX_DEGREE", _abi.SUR_MAX_DEGREE),
                            ("ERPL_SUR_MAX_ORDER", _abi.SUR_MAX_ORDER), ("ERPL_SUR_MAX_TERMS", _abi.SUR_MAX_TERMS),
                            ("ERPL_SUR_MAX_HOLDOUT", _abi.SUR_MAX_HOLDOUT)))
    assert _abi.ABI_VERSION == 4 and C.sizeof(_abi.ErplSurSpec) == 40


def test_new_symbols_are_declared_exported_and_documented(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def test_defaults_are_exact(lib):
    spec = _abi.ErplSurSpec()
    C.memset(C.byref(spec), 0xA5, C.sizeof(spec))
    assert lib.erpl_mc_surrogate_defaults(C.byref(spec)) == 0
    assert (spec.n_vars, spec.n_rows, list(spec.rows)) == (0, 3, [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, 0])
    assert (spec.degree, spec.order, spec.holdout, spec.reserved) == (2, 2, 0, 0)
    assert lib.erpl_mc_surrogate_defaults(None) == -1 and b"spec" in lib.erpl_mc_last_error()


def test_fit_refusals_come_before_any_device_work_in_the_documented_order(lib):
    good = bytes([N, U, N])
    bad_kinds = bytes([N, 2, N])

    def call(spec, factors=DUMMY, kinds=good, summary=DUMMY, extra=DUMMY, n=100, result=True, coef=DUMMY):
        res = _abi.ErplSurrogate()
        rc = lib.erpl_mc_surrogate(None, factors, kinds, summary, extra, None, n, C.byref(spec) if spec is not None else None,
                                   C.byref(res) if result else None, coef, None, None, None, None, None)
        return rc, lib.erpl_mc_last_error().decode()

    # every later check fails too: the earlier one has to be the one reported
    worst = dict(n_vars=0, n_rows=0, rows=(17, 17), degree=0, order=0, holdout=1)
    late = dict(kinds=bad_kinds, extra=None, n=0)
    # 1. NULL pointers, in the order of the arguments' list
    rc, msg = call(None, factors=None, kinds=None, summary=None, result=False, coef=None, n=0)
    assert rc == -1 and "spec" in msg
    for k, (name, gone) in enumerate((("factors", dict(factors=None)), ("kinds", dict(kinds=None)), ("summary", dict(summary=None)),
                                      ("result", dict(result=False)), ("coefficients", dict(coef=None)))):
        rest = {}
        for _, later in (("factors", dict(factors=None)), ("kinds", dict(kinds=None)), ("summary", dict(summary=None)),
                         ("result", dict(result=False)), ("coefficients", dict(coef=None)))[k:]:
            rest.update(later)
        rc, msg = call(spec_of(**worst), **dict(dict(extra=None, n=0), **rest))
        assert rc == -1 and name in msg and "NULL" in msg, (name, msg)
    # 2. n
    for n in (0, -3, 2 ** 31, 2 ** 40):
        rc, msg = call(spec_of(**worst), **dict(late, n=n))
        assert rc == -1 and f"n = {n}" in msg
    late = dict(kinds=bad_kinds, extra=None)
    # 3. n_vars, n_rows, degree, order, holdout
    fields = (("n_vars", (0, 33, -1), 3), ("n_rows", (0, 5), 2), ("degree", (0, 13), 11), ("order", (0, 5), 4), ("holdout", (1, -1, 2 ** 20 + 1), 2))
    fixed = dict(worst)
    for name, bads, ok in fields:
        for bad in bads:
            rc, msg = call(spec_of(**dict(fixed, **{name: bad})), **late)
            assert rc == -1 and name in msg and str(bad) in msg, (name, bad, msg)
        fixed[name] = ok
    # 4. a kind byte
    rc, msg = call(spec_of(**fixed), **late)
    assert rc == -1 and "kinds[1]" in msg
    # 5. a row out of range or listed twice
    for rows, what in (((17, 17), "rows[0]"), ((3, -1), "rows[1]"), ((16, 16), "twice")):
        rc, msg = call(spec_of(**dict(fixed, rows=rows)), extra=None)
        assert rc == -1 and what in msg, msg
    # 6. row 16 without extra
    rc, msg = call(spec_of(**dict(fixed, rows=(3, 16))), extra=None)
    assert rc == -1 and "extra" in msg
    # 7. P > 1024: (11, 4, 3) gives 1035
    rc, msg = call(spec_of(11, 2, (3, 16), 4, 3), kinds=bytes([U] * 11))
    assert rc == -1 and "1035" in msg and "ERPL_SUR_MAX_TERMS" in msg
    # 8. everything in order, at the limits: only the context is left
    for s, kinds in ((spec_of(25, 4, (0, 1, 2, 16), 3, 2, 2 ** 20), bytes([U, N] * 12 + [U])), (spec_of(32, 1, (16,), 12, 1, 0), bytes(32)),
                     (spec_of(1, 1, (15,), 1, 4, 2), bytes([N]))):
        rc, msg = call(s, kinds=kinds, n=2 ** 31 - 1)
        assert rc == -1 and "ctx" in msg, msg


@pytest.mark.parametrize("entry", ["device", "host"])
def test_predict_refusals_in_the_documented_order(lib, entry):
    good = bytes([N, U, N])

    def call(spec, kinds=good, coef=DUMMY, X=DUMMY, ld=100, n=100, out=DUMMY):
        sp = C.byref(spec) if spec is not None else None
        if entry == "device":
            rc = lib.erpl_mc_surrogate_predict(None, sp, kinds, coef, X, ld, n, out, None)
        else:
            rc = lib.erpl_mc_surrogate_predict_host(sp, kinds, coef, X, ld, n, out)
        return rc, lib.erpl_mc_last_error().decode()

    worst = dict(n_vars=0, n_rows=0, rows=(), degree=0, order=0)
    rc, msg = call(None, kinds=None, coef=None, X=None, out=None, n=0)
    assert rc == -1 and "spec" in msg
    gone = (("kinds", "kinds"), ("coefficients", "coef"), ("X", "X"), ("out", "out"))
    for k, (name, _) in enumerate(gone):
        rc, msg = call(spec_of(**worst), **dict({arg: None for _, arg in gone[k:]}, n=0, ld=-1))
        assert rc == -1 and name in msg and "NULL" in msg, (name, msg)
    for n in (0, -1, 2 ** 31):
        rc, msg = call(spec_of(**worst), kinds=bytes([N, 3, N]), n=n, ld=-1)
        assert rc == -1 and f"n = {n}" in msg
    fixed = dict(worst)
    for name, bads, ok in (("n_vars", (0, 33), 3), ("n_rows", (0, 5), 1), ("degree", (0, 13), 2), ("order", (0, 5), 2)):
        for bad in bads:
            rc, msg = call(spec_of(**dict(fixed, **{name: bad})), kinds=bytes([N, 3, N]), ld=5)
            assert rc == -1 and name in msg and str(bad) in msg
        fixed[name] = ok
    rc, msg = call(spec_of(**fixed), kinds=bytes([N, 3, N]), ld=5)
    assert rc == -1 and "kinds[1]" in msg
    rc, msg = call(spec_of(11, 1, (), 4, 3), kinds=bytes(11), ld=5)
    assert rc == -1 and "1035" in msg
    rc, msg = call(spec_of(**fixed), ld=99)
    assert rc == -1 and "ld" in msg
    if entry == "device":
        rc, msg = call(spec_of(**fixed))
        assert rc == -1 and "ctx" in msg


def _slices(length, P):
    """The tests' restatement of erpl_sur_slices / erpl_sur_max_slices: (slices, slice_len, most)."""
    tiles = -(-(P + 4) // 128)
    most = max(1, min(512 // (tiles * (tiles + 1) // 2), -(-length // 256)))
    per = -(-(-(-length // most)) // 16) * 16
    return -(-length // per), per, most


def test_workspace_layout_on_the_host(lib):
    """erpl_sur_layout through the table printer, before a kernel writes through an offset: every piece starts at a multiple
    of 256 behind the end of the piece before it, Psi holds cols rows of a chunk, and the partial tiles have room for the
    most slices the layout's chunk length allows."""
    subprocess.run(["make", "-s", "-C", CSRC, "erpl_stat_layout_table"], check=True)
    reqs = [(n, R, P) for n in (1, 9, 15, 16, 17, 300, 21760, 22000, 32768, 32769, 70010, 2 ** 20, 2 ** 31 - 1)
            for R, P in ((1, 2), (3, 13), (3, 276), (4, 396), (4, 561), (3, 976), (4, 1024))]
    text = "".join(f"sur {n} {R} {P} 1000\n" for n, R, P in reqs)
    r = subprocess.run([os.path.join(CSRC, "erpl_stat_layout_table")], input=text, capture_output=True, text=True, check=True)
    for (n, R, P), line in zip(reqs, r.stdout.splitlines()):
        pop, src, count, temp, model, psi, part, gram, yhat, temp_bytes, m_kinds, m_terms, m_coef, model_bytes, ld, slices, need = \
            map(int, line.split())
        cols, tiles = P + R, -(-(P + R) // 128)
        pairs = tiles * (tiles + 1) // 2
        sizes = [(pop, n), (src, 4 * n), (count, 8), (temp, temp_bytes), (model, model_bytes), (psi, 8 * cols * ld),
                 (part, 8 * slices * pairs * 128 * 128), (gram, 8 * cols * cols), (yhat, 8 * n * R)]
        at = 0
        for start, size in sizes:
            assert start % 256 == 0 and start >= at, (n, R, P, line)
            at = start + size
        assert need == at and temp_bytes >= 1000 and temp_bytes % 256 == 0
        assert ld % 16 == 0 and min(n, 32768) <= ld < min(n, 32768) + 16
        assert (m_kinds, m_terms, m_coef, model_bytes) == (4 * 8 * 13, 4 * 8 * 13 + 32, 4 * 8 * 13 + 32 + 8 * P, 4 * 8 * 13 + 32 + 8 * P + 8 * R * P)
        assert slices == _slices(ld, P)[2] and slices * pairs * 128 * 128 * 8 <= 64 << 20


@pytest.mark.parametrize("P", [2, 13, 124, 125, 276, 396, 561, 976, 1024])
def test_no_chunk_needs_more_slices_than_the_layout_has(lib, P):
    """Every chunk length from 1 to 32 768 + 15 (the longest `ld`): the library's slices equal the restatement's, cover the
    chunk with a slice length that is a multiple of 16, and are never more than erpl_sur_max_slices of ANY layout length at
    or above the chunk's - the room of the partial tiles.  The slice count itself is not monotone in the length: at P = 276 a
    chunk of 21 760 members has 85 slices and one of 22 000 has 81, which is what the layout must not be sized by."""
    subprocess.run(["make", "-s", "-C", CSRC, "erpl_stat_layout_table"], check=True)
    top = 32768 + 15
    # the library, one line per length; then the running maximum against the room at every length
    text = "".join(f"surslice {length} {P}\n" for length in range(1, top + 1))
    r = subprocess.run([os.path.join(CSRC, "erpl_stat_layout_table")], input=text, capture_output=True, text=True, check=True)
    got = np.array([[int(x) for x in line.split()] for line in r.stdout.splitlines()])
    want = np.array([_slices(length, P)[:2] for length in range(1, top + 1)])
    assert np.array_equal(got, want)
    length = np.arange(1, top + 1)
    assert np.all(got[:, 1] % 16 == 0) and np.all(got[:, 0] * got[:, 1] >= length) and np.all((got[:, 0] - 1) * got[:, 1] < length)
    room = np.array([_slices(ld, P)[2] for ld in range(1, top + 1)])
    assert np.all(np.diff(room) >= 0)                        # the room grows with the layout's length ..
    assert np.all(np.maximum.accumulate(got[:, 0]) <= room)  # .. and holds every chunk up to it
    # the same through the printer's own sweep, for the layout lengths the GPU cases and the bench use
    for ld in (16, 80, 272, 1200, 21760, 22000, 32768):
        out = subprocess.run([os.path.join(CSRC, "erpl_stat_layout_table")], input=f"surslices 1 {ld} {P}\n", capture_output=True,
                             text=True, check=True).stdout.split()
        most, _, have = int(out[0]), int(out[1]), int(out[2])
        assert 1 <= most <= have == _slices(ld, P)[2], (P, ld, out)
    if P == 276:
        assert _slices(21760, P)[0] == 85 and _slices(22000, P)[0] == 81 and _slices(22000, P)[2] == 85


def test_terms_refusals(lib):
    P = C.c_int32(0)
    assert lib.erpl_mc_surrogate_terms(3, 2, 2, None, None) == -1 and b"n_terms" in lib.erpl_mc_last_error()
    for args, name in (((0, 2, 2), "n_vars"), ((33, 2, 2), "n_vars"), ((3, 0, 2), "degree"), ((3, 13, 2), "degree"), ((3, 2, 0), "order"),
                       ((3, 2, 5), "order")):
        assert lib.erpl_mc_surrogate_terms(*args, C.byref(P), None) == -1 and name.encode() in lib.erpl_mc_last_error()
    assert lib.erpl_mc_surrogate_terms(11, 4, 3, C.byref(P), None) == -1 and b"1035" in lib.erpl_mc_last_error()
    assert R.count(11, 4, 3) == 1035


@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_terms_equal_the_reference_and_the_closed_form(lib, shape):
    tm = lib_terms(lib, *shape)
    ref = R.terms(*shape)
    assert len(tm) == SHAPES[shape] == R.count(*shape) == len(ref)
    assert np.array_equal(tm, ref)
    assert len({t.tobytes() for t in tm}) == len(tm)
    assert np.array_equal(tm[0], [[-1, 0]] * 4)


def test_the_header_alone_on_the_host():
    """csrc/erpl_pce_check: erpl_pce.h without the library - closed form against the enumeration, its order, no term twice,
    both bases orthonormal under Gauss quadrature."""
    subprocess.run(["make", "-s", "-C", CSRC, "erpl_pce_check"], check=True)     # (nothing to do after build())
    r = subprocess.run([os.path.join(CSRC, "erpl_pce_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok ") == 4 and "FAIL" not in r.stdout


def test_the_header_alone_under_a_host_sanitizer(tmp_path):
    """A second build of the same stand-alone program with TABFLAGS=-fsanitize=address,undefined, in a copy of the directory
    so that the product's build stays as it is.  Nothing of it is loaded into Python."""
    csrc = tmp_path / "pkg" / "csrc"
    csrc.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    for name in ("Makefile", "erpl_pce_check.cpp", "erpl_pce.h"):
        shutil.copy(os.path.join(CSRC, name), csrc / name)
    shutil.copy(os.path.join(REPO, "include", "erpl_mc.h"), tmp_path / "include" / "erpl_mc.h")
    subprocess.run(["make", "-s", "-C", str(csrc), "erpl_pce_check", "TABFLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all"],
                   check=True)
    r = subprocess.run([str(csrc / "erpl_pce_check")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("ok ") == 4, r.stdout + r.stderr


def _random_model(rng, shape, n_rows=2):
    n_vars, degree, order = shape
    kinds = [N if (v + n_vars) % 2 == 0 else U for v in range(n_vars)]
    coef = rng.normal(size=(n_rows, SHAPES[shape])) * np.exp(rng.normal(size=(n_rows, SHAPES[shape])))
    return kinds, coef


def _inputs(rng, kinds, n):
    X = np.empty((len(kinds), n))
    for v, k in enumerate(kinds):
        X[v] = rng.uniform(-8.0, 8.0, n) if k == N else rng.uniform(0.0, 1.0, n)
        edge = (-8.0, 8.0, 0.0, -0.0) if k == N else (2.0 ** -53, 1.0 - 2.0 ** -53, 0.5, 2.0 ** -53)
        X[v, :4] = np.roll(edge, v)
    return X


@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_predict_host_equals_the_reference_bit_for_bit(lib, shape):
    """Random models with coefficients over several orders of magnitude, mixed kinds, |z| up to 8, u at 2^-53 and 1 - 2^-53;
    NaN and inf inputs give NaN; with n < ld the columns from n on are left as they are."""
    rng = np.random.default_rng(hash(shape) % 2 ** 32)
    kinds, coef = _random_model(rng, shape)
    X = _inputs(rng, kinds, 203)
    X[0, 17], X[-1, 40], X[0, 41] = np.nan, np.inf, -np.inf
    n_vars, degree, order = shape
    want = R.predict(kinds, degree, R.terms(*shape), coef, X)
    got = host_predict(lib, kinds, degree, order, coef, X)
    assert np.all(np.isnan(got[:, [17, 40, 41]])) and np.isfinite(np.delete(got, [17, 40, 41], axis=1)).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.all(np.isnan(want) | (got.view(np.uint64) == want.view(np.uint64)))
    part = host_predict(lib, kinds, degree, order, coef, X, n=150)
    assert np.array_equal(part[:, :150], got[:, :150], equal_nan=True) and np.all(part[:, 150:] == -7.0)


def test_the_reference_reproduces_ishigami(lib):
    """4096 uniform points, degree 10, order 3 (286 terms): every analytic index, mean / 3.5 and variance / 13.8446 within
    2e-3; x3 has no first-order effect but a total one, all of it through the pair (x1, x3)."""
    rng = np.random.default_rng(20240607)
    Uu = rng.uniform(size=(3, 4096))
    x = np.pi * (2.0 * Uu - 1.0)
    y = R.ishigami(*x)
    tm, coef, _, cond = R.fit([U, U, U], Uu, y, 10, 3)
    assert len(tm) == 286 and cond < 1e3
    mean, var, first, total, pair = R.derived(coef[0], tm, 3)
    a_mean, a_var, a_first, a_total, a_13 = R.ishigami_analytic()
    print(f"cond {cond:.1f}; mean {mean / a_mean - 1:.2e} var {var / a_var - 1:.2e} first {np.abs(first - a_first).max():.2e} "
          f"total {np.abs(total - a_total).max():.2e} pair13 {abs(pair[0, 2] - a_13):.2e}")
    assert abs(a_var - 13.8446) < 1e-4
    assert abs(mean / a_mean - 1.0) <= 2e-3 and abs(var / a_var - 1.0) <= 2e-3
    assert np.all(np.abs(first - a_first) <= 2e-3) and np.all(np.abs(total - a_total) <= 2e-3)
    assert first[2] < 1e-3 and abs(total[2] - 0.2437) <= 2e-3 and abs(pair[0, 2] - total[2]) <= 2e-3 and pair[0, 2] == pair[2, 0]
    assert abs(pair[0, 1]) <= 2e-3 and abs(pair[1, 2]) <= 2e-3
    # the library's own evaluation of that model at new points: a variance within 2e-3 leaves an rms error of about
    # sqrt(2e-3) = 0.045 standard deviations at the most
    Xn = rng.uniform(size=(3, 4096))
    got = host_predict(lib, [U, U, U], 10, 3, coef, Xn)[0]
    rms = np.sqrt(np.mean((got - R.ishigami(*(np.pi * (2.0 * Xn - 1.0)))) ** 2))
    print(f"rms error of the emulator at new points: {rms / np.sqrt(a_var):.4f} standard deviations")
    assert rms <= 0.05 * np.sqrt(a_var)


def test_the_reference_gives_nan_indices_for_a_zero_variance():
    """variance_pce == 0 (every coefficient but the constant's zero): the mean stays, every index is NaN."""
    tm = R.terms(3, 2, 2)
    mean, var, first, total, pair = R.derived(np.array([7.25] + [0.0] * (len(tm) - 1)), tm, 3)
    assert mean == 7.25 and var == 0.0 and np.all(np.isnan(first)) and np.all(np.isnan(total)) and np.all(np.isnan(pair))
    mean, var, first, total, pair = R.derived(np.array([0.0, 2.0] + [0.0] * (len(tm) - 2)), tm, 3)
    assert var == 4.0 and first.tolist() == [1.0, 0.0, 0.0] and total.tolist() == [1.0, 0.0, 0.0] and np.all(pair == 0.0)


def test_engine_refuses_host_tensors():
    """No CPU path behind TrajectoryEngine.surrogate / surrogate_predict: the refusal is on the host, before the library."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    eng.lib = H.load_lib()
    with pytest.raises(ValueError, match="summary"):
        TrajectoryEngine.surrogate(eng, torch.zeros((2, 8), dtype=torch.float64), [N, U], torch.zeros((16, 8), dtype=torch.float64))
    model = {"kinds": bytes([N, U]), "degree": 2, "order": 2, "coefficients": np.zeros((1, 6))}
    with pytest.raises(ValueError, match="X"):
        TrajectoryEngine.surrogate_predict(eng, model, torch.zeros((2, 8), dtype=torch.float64))
