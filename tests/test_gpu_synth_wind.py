"""erpl_mc_synth_wind (the erpl_wind_ar1 kernel) through the C ABI, value for value: every element of the table against the
long-double restatement of the header's formula (tests/synth_wind_ref.py) within 8 eps E, with per-knot constants that
differ at every knot so that an index slip moves the result; the exact identities of the kernel (zero normals, base of
zeros, the fp32 table as the rounding of the fp64 one), the footprint of a single normal, guard bands round the output,
the refusals, the stream argument, and the reference's own MT19937 normals and constants through the device kernel
against the table flatten.dispersed_batch builds (bit-equal to the reference's)."""
import ctypes as C

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, flatten, models

import helpers as H
import synth_wind_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256
PATTERN32 = 0x7FC0DE01                       # a float32 NaN with a payload
PATTERN = PATTERN32 << 32 | PATTERN32        # as a double 5e306: no wind has either
F64, F32, F64_FAST = _abi.PREC_F64, _abi.PREC_F32, _abi.PREC_F64_FAST

# each n and each K at least once, paired, not the product: 3 n = 255 and 258 straddle one 256-thread workgroup (n = 85,
# 86), 64 +- 1 a wave; K = 1024 is ERPL_MAX_WIND_KNOTS
SHAPES = [(1, 1), (2, 2), (63, 3), (64, 6), (65, 100), (85, 1024), (86, 1), (255, 2), (256, 3), (257, 6), (1000, 100),
          (1000, 1024)]


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def upload(engine, v):
    return None if v is None else torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=engine.device)


def guarded(engine, numel, dtype):
    """A buffer of GUARD + numel + GUARD elements filled with the pattern, and its middle."""
    idt, pat = (torch.int32, PATTERN32) if dtype == torch.float32 else (torch.int64, PATTERN)
    buf = torch.full((GUARD + numel + GUARD,), pat, dtype=idt, device=engine.device).view(dtype)
    return buf, buf[GUARD:GUARD + numel]


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def untouched(buf):
    return bool((bits(buf) == (PATTERN32 if buf.dtype == torch.float32 else PATTERN)).all())


def all_written(wind):
    return not bool((bits(wind) == (PATTERN32 if wind.dtype == torch.float32 else PATTERN)).any())


def call(engine, n, K, dev, wind, precision=F64, stream=None):
    """The call of sampling.synthetic_dispersions; dev = (normals, sigma, rho, innov, base, scale, mean_u, mean_v)."""
    st = torch.cuda.current_stream(engine.device) if stream is None else stream
    rc = engine.lib.erpl_mc_synth_wind(engine._ctx, n, K, *[ptr(t) for t in dev], ptr(wind), int(precision),
                                       C.c_void_p(st.cuda_stream))
    return rc


def synth(engine, args, precision=F64):
    """The table [K, 3, n] of host inputs `args` (the argument list of R.reference) as a NumPy array, written between guard
    bands that are checked here."""
    z, sigma = np.asarray(args[0]), np.asarray(args[1])
    K, n = len(sigma), len(args[6])
    dev = [upload(engine, v) for v in args]
    dev[0] = dev[0].reshape(K, 3, n)
    dt = torch.float32 if precision == F32 else torch.float64
    buf, wind = guarded(engine, K * 3 * n, dt)
    assert call(engine, n, K, dev, wind, precision) == R.OK, engine.lib.erpl_mc_last_error()
    torch.cuda.synchronize()
    assert untouched(buf[:GUARD]) and untouched(buf[GUARD + K * 3 * n:]), "a write outside the table"
    assert all_written(wind), "an element of the table was not written"
    return wind.cpu().numpy().reshape(K, 3, n)


def hand_made(K, n, with_base=True, seed=None):
    seed = 1000 * K + n if seed is None else seed
    sigma, rho, innov, scale, base = R.knot_inputs(seed, K)
    z, mu, mv = R.sample_inputs(seed + 1, K, n)
    return [z, sigma, rho, innov, base if with_base else None, scale, mu, mv]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ value for value
@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("n,K", SHAPES)
def test_every_element_is_the_formula_of_the_header(engine, n, K, with_base):
    """Measured on the MI355X: 0.33 (n = 1, K = 1) to 1.23 eps E (n = 1000, K = 1024) against the 8 eps E asserted."""
    args = hand_made(K, n, with_base)
    got = synth(engine, args)
    x = R.excess(got, R.reference(*args), R.bound(*args))
    print(f"n = {n}, K = {K}, base {with_base}: {x:.2f} eps E")
    assert got.dtype == np.float64 and x <= R.TOL


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("n,K", [(86, 6), (257, 100)])
def test_exact_identities(engine, n, K):
    args = hand_made(K, n, with_base=False)
    z, scale, mu, mv = args[0], args[5], args[6], args[7]
    # zero normals, no base: the mean wind alone, and no vertical wind at all
    still = list(args)
    still[0] = np.zeros_like(z)
    got = synth(engine, still)
    assert same_bits(got[:, 0], scale[:, None] * mu[None, :]) and same_bits(got[:, 1], scale[:, None] * mv[None, :])
    assert same_bits(got[:, 2], np.zeros((K, n)))
    # a base of zeros is no base
    a = synth(engine, args)
    zeros = list(args)
    zeros[4] = np.zeros((K, 3))
    assert same_bits(synth(engine, zeros), a)
    # the same call twice
    assert same_bits(synth(engine, args), a)
    # the recursion runs in fp64 whatever the table's type; F64_FAST is a flight-kernel build, not another table
    with_base = hand_made(K, n, with_base=True)
    b = synth(engine, with_base)
    f = synth(engine, with_base, F32)
    assert f.dtype == np.float32 and same_bits(f, b.astype(np.float32))
    assert same_bits(synth(engine, with_base, F64_FAST), b)
    assert same_bits(synth(engine, args, F64_FAST), a) and same_bits(synth(engine, args, F32), a.astype(np.float32))


# ------------------------------------------------------------------ footprint of one normal
# n = 86, K = 6: threads 0..255 of workgroup 0 hold components 0, 1 and samples 0..83 of component 2; workgroup 1 holds
# samples 84, 85 of component 2
@pytest.mark.parametrize("j,c,s", [(0, 0, 0), (2, 1, 40), (5, 0, 85), (1, 2, 83), (3, 2, 84), (0, 2, 85)])
def test_one_normal_moves_its_own_column_from_its_knot_on(engine, j, c, s):
    n, K = 86, 6
    args = hand_made(K, n)
    a = synth(engine, args)
    moved = list(args)
    moved[0] = args[0].copy()
    moved[0][j, c, s] += 1.0
    b = synth(engine, moved)
    differs = a.view(np.int64) != b.view(np.int64)
    want = np.zeros((K, 3, n), dtype=bool)
    want[j:, c, s] = True
    assert np.array_equal(differs, want)
    assert R.excess(b, R.reference(*moved), R.bound(*moved)) <= R.TOL


# ------------------------------------------------------------------ no stray writes, nothing to do, refusals
@pytest.mark.parametrize("precision", [F64, F32])
def test_nothing_to_do_and_refusals_leave_the_buffer_alone(engine, precision):
    n, K = 85, 6
    args = hand_made(K, n)
    dev = [upload(engine, v) for v in args]
    dt = torch.float32 if precision == F32 else torch.float64
    buf, wind = guarded(engine, K * 3 * n, dt)
    lib = engine.lib

    def check(rc, want, what):
        torch.cuda.synchronize()
        assert rc == want, (what, rc, lib.erpl_mc_last_error())
        assert untouched(buf), what

    check(call(engine, 0, K, dev, wind, precision), R.OK, "n = 0")
    check(call(engine, n, 0, dev, wind, precision), R.OK, "k = 0")
    check(call(engine, 0, 0, [None] * 8, None, precision), R.OK, "n = k = 0 without buffers")
    # 1025 knots: the constants really are that long, so that a call that went through would not read out of bounds
    long_ = [upload(engine, v) for v in hand_made(_abi.MAX_WIND_KNOTS + 1, 1)]
    big, big_wind = guarded(engine, (_abi.MAX_WIND_KNOTS + 1) * 3, dt)
    rc = call(engine, 1, _abi.MAX_WIND_KNOTS + 1, long_, big_wind, precision)
    torch.cuda.synchronize()
    assert rc == R.ERR_INVALID and untouched(big)
    check(call(engine, -1, K, dev, wind, precision), R.ERR_INVALID, "n = -1")
    check(call(engine, n, -1, dev, wind, precision), R.ERR_INVALID, "k = -1")
    for bad in (3, -1, 7):
        check(call(engine, n, K, dev, wind, bad), R.ERR_INVALID, f"precision {bad}")
    names = ("normals", "sigma", "rho", "innov", "base", "scale", "mean_u", "mean_v")
    for i, name in enumerate(names):
        if name == "base":
            continue
        holed = list(dev)
        holed[i] = None
        check(call(engine, n, K, holed, wind, precision), R.ERR_INVALID, f"{name} = NULL")
    check(call(engine, n, K, dev, None, precision), R.ERR_INVALID, "wind = NULL")
    st = torch.cuda.current_stream(engine.device)
    rc = lib.erpl_mc_synth_wind(None, n, K, *[ptr(t) for t in dev], ptr(wind), int(precision), C.c_void_p(st.cuda_stream))
    check(rc, R.ERR_INVALID, "ctx = NULL")
    # and the buffer is a live one: the same arguments, unrefused, fill exactly the table
    assert call(engine, n, K, dev, wind, precision) == R.OK
    torch.cuda.synchronize()
    assert untouched(buf[:GUARD]) and untouched(buf[GUARD + K * 3 * n:]) and all_written(wind)


# ------------------------------------------------------------------ stream
def test_the_call_is_ordered_on_the_stream_it_is_given(engine):
    """Inputs that are filled ON a side stream, behind work that keeps that stream busy, are what the kernel reads: it is
    enqueued on that stream, not on the default one (where it would find the stale zeros)."""
    n, K = 1000, 100
    args = hand_made(K, n)
    host = [None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).pin_memory() for v in args]
    dev = [torch.zeros(h.shape, dtype=torch.float64, device=engine.device) for h in host]
    buf, wind = guarded(engine, K * 3 * n, torch.float64)
    busy = torch.ones((1 << 24,), dtype=torch.float64, device=engine.device)
    side = torch.cuda.Stream(engine.device)
    torch.cuda.synchronize()
    assert side.cuda_stream != torch.cuda.current_stream(engine.device).cuda_stream
    with torch.cuda.stream(side):
        for _ in range(24):
            busy.mul_(1.0)
        for d, h in zip(dev, host):
            d.copy_(h, non_blocking=True)
        assert call(engine, n, K, dev, wind, F64, stream=side) == R.OK
    torch.cuda.current_stream(engine.device).wait_stream(side)
    got = wind.clone().cpu().numpy().reshape(K, 3, n)
    assert untouched(buf[:GUARD]) and untouched(buf[GUARD + K * 3 * n:])
    assert R.excess(got, R.reference(*args), R.bound(*args)) <= R.TOL


# ------------------------------------------------------------------ the reference's own tables through the device kernel
@pytest.mark.parametrize("csv", [True, False], ids=["csv_k6", "synthetic_k100"])
def test_the_reference_wind_tables_through_the_device_kernel(engine, csv):
    """MT19937 normals of seeds 0..n-1, the per-knot constants as flatten.legacy_wind_profiles prepares them and the mean
    rows of generate_parameter_arrays, fed to erpl_mc_synth_wind: the table flatten.dispersed_batch builds (bit-equal to
    the reference's own, tests/test_host.py) within 8 eps E.  Ties the throughput kernel to the reference's wind model, not
    only to the header's prose."""
    n, wm = 257, models.WindModel()
    seeds = np.arange(n, dtype=np.uint32)
    P = flatten.generate_parameter_arrays(H.UNCERTAINTY, n)
    kw = dict(base_altitude_profile=H.CSV_ALT, base_wind_profile=H.CSV_WIND) if csv else {}
    hb = flatten.dispersed_batch(models.Rocket(), models.LiquidMotor(), wm, H.EXAMPLE_IC, P, **kw)
    alt = hb.alt_grid
    K = len(alt)
    assert K == (6 if csv else 100)
    g = flatten.legacy_streams(seeds, "g" * (3 * K), by_output=True)
    sigma, rho, innov = models.knot_constants(wm, alt)
    rho, innov = [0.0] + list(rho[1:]), [0.0] + list(innov[1:])
    if csv:
        base, scale = np.asarray(H.CSV_WIND, dtype=np.float64), np.ones(K)
    else:
        base, scale = None, np.array([(np.float64(a) / 10.0) ** wm.power_law_exponent for a in alt])
    speed, direction = P["wind_speed"], P["wind_direction"]
    args = [g, sigma, rho, innov, base, scale, speed * np.cos(direction), speed * np.sin(direction)]
    got = synth(engine, args)
    E = R.bound(*args)
    x, y = R.excess(got, hb.wind, E), R.excess(got, R.reference(*args), E)
    print(f"K = {K}: device - dispersed_batch {x:.2f} eps E, device - long double {y:.2f} eps E")
    assert x <= R.TOL and y <= R.TOL
