"""The fp64 throughput build after the second diet of its RK4 step: the bits of mixed waves, and the single-instruction
max / min / clamp forms on the device.

tests/golden/step_diet_bits_*.npy were recorded by tools/record_step_diet_bits.py with the library of the parent commit: before
the force and moment sums were set on every path instead of zero-initialised, before v_max_f64 / v_min_f64 lost their quieting
moves and before the running speed maximum became one v_max_f64.  The batches are those of step_diet_cases.py: in every wave of 64 lanes
some have the parachute out and some not, one is at rest relative to the wind while the others fly, some burn and some have
burnt out, some tumble past the hand-over speed and turn non-finite.  No tolerance: every value and every status word, through
erpl_mc_run_batch and as a submitted batch (the parent returned the same bytes both ways: one file per size).

The max / min / clamp forms are compared with numpy.fmax / numpy.fmin bit for bit (a NaN equals a NaN), through
erpl_mc_debug_eval(ERPL_DBG_MINMAX) - the very device functions the flight kernel inlines, with every kind of second operand
they take there: a vector register, the inline constants, a constant through a scalar register pair, a kernel argument.
One deviation from "numpy, bit for bit": +0 against -0, where numpy's answer depends on the operand order (fmax_ref below).
A signalling NaN, the one input on which the instruction and fmax / fmin differ, has a test of its own."""
import os

import numpy as np
import pytest
import torch

import helpers as H
import step_diet_cases as cases
from erpl_monte_carlo_sim_amd import _abi, flatten, models

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def golden(n):
    path = os.path.join(H.GOLDEN, cases.file_name(n))
    assert os.path.getsize(path) <= 64 * 1024
    a = np.load(path)
    assert a.shape == (2, 17, n) and a.dtype == np.float64 and np.all(np.isfinite(a))
    return a


def decode(enc):
    """[2, 17, n] finite values + markers -> the [17, n] array with its NaN and infinities."""
    flight = enc[0].copy()
    for mark, v in ((1.0, np.nan), (2.0, np.inf), (3.0, -np.inf)):
        flight[enc[1] == mark] = v
    return flight


@pytest.mark.parametrize("n", cases.SIZES)
def test_every_wave_of_the_recording_is_mixed(n):
    assert cases.missing(decode(golden(n))) == []


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("n", cases.SIZES)
def test_same_bits_as_recorded(engine, n, mode):
    got, want = cases.encode(cases.collect(engine, n, mode)), golden(n)
    # (the encoded arrays hold finite numbers only; -0.0 == 0.0 would pass array_equal, so the comparison is on the bytes)
    same = got.shape == want.shape and got.tobytes() == want.tobytes()
    if not same and got.shape == want.shape:
        bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
        print("%d %s: %d of %d values differ, first at %s: %r != %r" % (
            n, mode, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))
    assert same, (n, mode)


# ------------------------------------------------------------------------------------ the max / min / clamp forms
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308,
                     2.2250738585072014e-308, 1e-30, np.nextafter(1e-30, 0.0), np.nextafter(1e-30, 1.0), -1e-30, 1.0, -1.0,
                     np.nextafter(1.0, 2.0), np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), 0.5, -0.5, 0.2617993877991494,
                     -0.2617993877991494, 0.3, -0.3, 2.0, -2.0, 1e30, -1e30, np.nextafter(1e30, np.inf), np.nextafter(-1e30, -np.inf),
                     1.7976931348623157e308, -1.7976931348623157e308, 3.141592653589793, -123456.789])


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def minmax(engine):
    """-> (x, y, z, out [ERPL_DBG_MINMAX_ROWS, m], stall angle): every pair of SPECIALS as (x, y), z cycling through them."""
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    cfg = H.make_config("liquid")
    engine.set_config(cfg)
    hb = flatten.HostBatch(1, 0)
    r = models.Rocket()
    hb.rocket[:, 0] = [r.dry_mass, r.propellant_mass]
    hb.motor[:, 0] = flatten.motor_row(H.make_motor("liquid"))
    hb.ic[6, 0] = 1.0
    db = DeviceBatch.from_host(hb, engine.device, _abi.PREC_F64_FAST)
    x, y = [a.ravel() for a in np.meshgrid(SPECIALS, SPECIALS)]
    z = np.roll(np.resize(SPECIALS, x.size), 3)
    out = engine.debug_eval(db, _abi.DBG_MINMAX, np.stack([x, y, z]))
    assert out.shape == (_abi.DBG_MINMAX_ROWS, x.size)
    return x, y, z, out, 15.0 * (np.pi / 180.0)      # the stall angle as the host computes it (rocket.py:167-168)


def _mixed_zeros(a, b):
    return (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))


def fmax_ref(a, b):
    """numpy.fmax, except on +0 against -0: there IEEE 754 leaves the choice open, numpy returns one or the other depending on
    the operand order and on the code path its CPU dispatch picks, and v_max_f64 orders -0 below +0 (as maximumNumber of
    IEEE 754-2019 does).  That one pair is held to the instruction's documented order instead."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return np.where(_mixed_zeros(a, b), 0.0, np.fmax(a, b))


def fmin_ref(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return np.where(_mixed_zeros(a, b), -0.0, np.fmin(a, b))


def check(name, got, want, x, y):
    ok = same_bits(got, want)
    if not ok.all():
        bad = np.flatnonzero(~ok)
        print("%s: %d of %d differ, first at x = %r, y = %r: %r != %r" % (name, bad.size, got.size, x[bad[0]], y[bad[0]],
                                                                         got[bad[0]], want[bad[0]]))
    assert ok.all(), name


def test_max_min_clamp_against_numpy(minmax):
    x, y, z, out, _ = minmax
    assert _mixed_zeros(x, y).sum() == 2 and np.isnan(x).any() and np.isnan(y).any() and (np.isnan(x) & np.isnan(y)).any()
    check("m_max", out[0], fmax_ref(x, y), x, y)
    check("m_min", out[1], fmin_ref(x, y), x, y)
    check("m_clamp", out[2], fmin_ref(fmax_ref(x, y), z), x, y)


def test_constant_and_uniform_second_operands(minmax):
    x, y, _, out, stall = minmax
    check("m_max(x, 0)", out[3], fmax_ref(x, 0.0), x, y)
    check("m_max(x, 1e-30)", out[4], fmax_ref(x, 1e-30), x, y)
    check("m_clamp(x, -kBig, kBig)", out[5], fmin_ref(fmax_ref(x, -1e30), 1e30), x, y)
    check("m_clamp_abs_uniform", out[6], fmin_ref(fmax_ref(np.abs(x), -1.0), stall), x, y)
    check("m_add_zero", out[7], 0.0 + x, x, y)
    assert not np.signbit(out[7][x == 0]).any()      # 0 + -0 = +0: what the addition is kept for


def test_a_signalling_nan_comes_back_quiet(engine):
    """The one input on which the instruction differs from fmax / fmin: those drop a signalling NaN beside a number (they
    quiet it first, then return the number), v_max_f64 / v_min_f64 in IEEE mode return it quieted.  No arithmetic instruction
    produces one and the host refuses non-finite inputs, so no flight can tell; this pins what the forms do."""
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    hb = flatten.HostBatch(1, 0)
    r = models.Rocket()
    hb.rocket[:, 0] = [r.dry_mass, r.propellant_mass]
    hb.motor[:, 0] = flatten.motor_row(H.make_motor("liquid"))
    hb.ic[6, 0] = 1.0
    db = DeviceBatch.from_host(hb, engine.device, _abi.PREC_F64_FAST)
    s1, s2 = 0x7FF0000000000001, 0xFFF4000000000000      # quiet bit (51) clear, payload not zero
    two, one, mthree, mone = (int(np.float64(v).view(np.uint64)) for v in (2.0, 1.0, -3.0, -1.0))
    x = np.array([s1, two, s2, mthree], dtype=np.uint64).view(np.float64)
    y = np.array([one, s1, mone, s2], dtype=np.uint64).view(np.float64)
    assert ((np.stack([x, y]).view(np.uint64) & np.uint64(0x7FF8000000000000)) == np.uint64(0x7FF0000000000000)).sum() == 4
    engine.set_config(H.make_config("liquid"))
    out = engine.debug_eval(db, _abi.DBG_MINMAX, np.stack([x, y, np.ones(4)]))
    quiet = np.uint64(0x0008000000000000)
    for row in (0, 1):
        bits = out[row].view(np.uint64)
        assert np.isnan(out[row]).all() and ((bits & quiet) != 0).all(), (row, [hex(int(b)) for b in bits])
