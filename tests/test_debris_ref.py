"""tests/debris_ref.py, the NumPy restatement of erpl_mc_debris, checked on the CPU before the GPU tests lean on it: against
the closed form of a fall without drag or wind, against the restatement of erpl_mc_impact_points where the two must agree to
the bit, on the stiff falls the step rule exists for, and its directions against the library's host export."""
import math

import numpy as np
import pytest

from erpl_monte_carlo_sim_amd import _abi, analysis

import helpers as H
import debris_ref
import iip_ref
from test_iip_ref import mc_batch

A = _abi
INF = float("inf")

# The stiff falls of DESIGN.md 8.18: (z0, v0, beta), no impulse, dt = 0.25, the oracle's wind of sample 0.
STIFF = ((500.0, (250.0, 0.0, 100.0), 2.0), (500.0, (250.0, 0.0, 100.0), 10.0), (3000.0, (600.0, 0.0, 300.0), 50.0),
         (20000.0, (300.0, 0.0, 400.0), 2.0))
# Relative errors of dt = 0.25 against dt / 8, both under the step rule at 0.25, measured here with wind (printed by the test;
# DESIGN.md 8.18 has the table): the worst is 1.6e-5 in X (3 km, beta 50) and 2.97e-6 in TFALL
# (500 m, beta 10).  The bars are ten times those, to cover
# the cases not sampled.
X_WORST, T_WORST = 1.6e-5, 2.97e-6
X_BAR, T_BAR = 10.0 * X_WORST, 10.0 * T_WORST


@pytest.fixture(scope="module")
def world(oracle):
    cfg, hb = H.make_config("liquid"), mc_batch("liquid", 8, True)
    iip_ref.mass_cg_index(oracle, cfg)
    return cfg, hb


def record(x, y, z, v, pf=0.3):
    rec = np.zeros(15)
    rec[1:7] = (x, y, z) + tuple(v)
    rec[14] = pf
    return rec


def test_no_drag_no_wind_is_the_parabola(oracle, world):
    """beta = inf, no impulse, no wind: the cases and the 1e-4 bars of test_iip_ref.py, for the derivation given there (g
    varies by at most 3.2e-5 over 100 m, RK4 is exact for the parabola, the chord of the last step adds at most 5.1e-5)."""
    cfg, hb = world
    fall = debris_ref.Fall(oracle, cfg, hb.take([0]), dt=0.05, max_steps=4000, wind=False)
    g0 = float(cfg.gravity)
    for z0, v in ((100.0, (30.0, -4.0, 0.0)), (100.0, (5.0, 2.0, 40.0)), (60.0, (0.0, 0.0, -10.0)), (12.5, (80.0, 0.0, 15.0)),
                  (30.0, (3.0, 1.0, 0.0))):
        x, y, rng, tfall, vimp = fall.job(record(10.0, -20.0, z0, v), 0, 0, INF, 0.0)
        t = (v[2] + math.sqrt(v[2] * v[2] + 2.0 * g0 * z0)) / g0
        assert abs(v[2] - g0 * t) * t >= 60.0
        assert abs(tfall - t) <= 1e-4 * t, (z0, v, tfall, t)
        for got, x0, vx in ((x, 10.0, v[0]), (y, -20.0, v[1])):
            assert abs((got - x0) - vx * t) <= 1e-4 * max(abs(vx * t), 1e-9), (z0, v, got)
        assert abs(vimp - math.sqrt(v[0] ** 2 + v[1] ** 2 + (v[2] - g0 * t) ** 2)) <= 1e-4 * vimp
        assert rng == math.sqrt(x * x + y * y) and fall.steps - 1 <= tfall / 0.05 <= fall.steps and fall.max_m == 0
    # the node rules: at or below the ground, not of physical size (after the impulse), a fall that max_steps cuts short
    rec = record(3.0, 4.0, 0.0, (1.0, 2.0, -2.0))
    assert fall.job(rec, 0, 0, INF, 0.0) == [3.0, 4.0, 5.0, 0.0, 3.0]
    assert all(math.isnan(v) for v in fall.job(record(0.0, 0.0, 50.0, (0.0, 0.0, 2e6)), 0, 0, 5.0, 0.0))
    assert all(math.isnan(v) for v in fall.job(record(0.0, 0.0, -2e5, (0.0, 0.0, 0.0)), 0, 0, 5.0, 0.0))
    d = debris_ref.direction(0, 0, 0, 0)
    rec_up = record(0.0, 0.0, -1.0, tuple((1e6 - 50.0) * c for c in d))   # the impulse of 100 m/s along d carries it past 1e6
    assert not math.isnan(fall.job(rec_up, 0, 0, INF, 0.0)[0]) and all(math.isnan(v) for v in fall.job(rec_up, 0, 0, INF, 100.0))
    short = debris_ref.Fall(oracle, cfg, hb.take([0]), dt=0.05, max_steps=10, wind=False)
    assert all(math.isnan(v) for v in short.job(record(0.0, 0.0, 100.0, (0.0, 0.0, 0.0)), 0, 0, INF, 0.0)) and short.steps == 10


def test_no_drag_no_impulse_equals_the_impact_point_restatement(oracle, world):
    """beta = inf and dv = 0: k = 0 / inf = 0 where iip_ref has cd * 0 = 0, no step is halved, the ticks give (n + wq) * dt:
    the five channels are EQUAL, with wind and without, at two steps."""
    cfg, hb = world
    for sid, dt, wind in ((0, 0.05, True), (3, 0.25, True), (5, 0.1, False)):
        deb = debris_ref.Fall(oracle, cfg, hb.take([sid]), sid=sid, dt=dt, max_steps=4000, wind=wind)
        iip = iip_ref.Fall(oracle, cfg, hb.take([sid]), dt=dt, max_steps=4000, drag_scale=0.0, wind=wind)
        for z0, v in ((100.0, (30.0, -4.0, 0.0)), (1500.0, (250.0, 3.0, 120.0)), (12.5, (80.0, 0.0, 15.0)), (-3.0, (1.0, 2.0, 3.0))):
            rec = record(10.0, -20.0, z0, v)
            got, want = deb.job(rec, 2, 1, INF, 0.0), iip.node(rec)
            assert got == want and deb.max_m == 0 and deb.steps == iip.steps, (sid, z0, got, want)


def test_stiff_falls_land_where_the_fine_step_says(oracle, world):
    cfg, hb = world
    hb1 = hb.take([0])
    worst_x = worst_t = 0.0
    for z0, v, beta in STIFF:
        rec = record(0.0, 0.0, z0, v)
        coarse = debris_ref.Fall(oracle, cfg, hb1, dt=0.25, max_steps=1 << 20)
        fine = debris_ref.Fall(oracle, cfg, hb1, dt=0.25 / 8.0, max_steps=1 << 20)
        fixed = debris_ref.Fall(oracle, cfg, hb1, dt=0.25, max_steps=1 << 20, adaptive=False)
        c, steps, m = coarse.job(rec, 0, 0, beta, 0.0), coarse.steps, coarse.max_m
        f = fine.job(rec, 0, 0, beta, 0.0)
        x = fixed.job(rec, 0, 0, beta, 0.0)
        ex = abs(c[A.IIP_CH_X] - f[A.IIP_CH_X]) / abs(f[A.IIP_CH_X])
        et = abs(c[A.IIP_CH_TFALL] - f[A.IIP_CH_TFALL]) / f[A.IIP_CH_TFALL]
        print(f"z0 {z0:g} v {v} beta {beta:g}: fixed step X {x[A.IIP_CH_X]:.6g} after {fixed.steps} steps | rule X {c[A.IIP_CH_X]:.9g} "
              f"TFALL {c[A.IIP_CH_TFALL]:.9g} in {steps} steps, largest m {m} | dt/8 X {f[A.IIP_CH_X]:.9g} TFALL {f[A.IIP_CH_TFALL]:.9g} "
              f"| relative error X {ex:.3g} TFALL {et:.3g}")
        worst_x, worst_t = max(worst_x, ex), max(worst_t, et)
        assert ex <= X_BAR and et <= T_BAR, (z0, v, beta, ex, et)
        if z0 == 500.0 and beta == 2.0:
            # a fixed-step fall overshoots through the ground in its first step and reports a landing behind the start
            assert c[A.IIP_CH_X] > 0.0 and steps > 100 and m == 7, (c, steps, m)
            assert fixed.steps <= 2 and x[A.IIP_CH_X] < 0.0, (x, fixed.steps)
    print(f"worst relative error: X {worst_x:.3g} TFALL {worst_t:.3g}")


def test_directions_equal_the_host_export_and_are_isotropic():
    lib = H.load_lib()
    assert lib is not None
    n = 4096
    ids = np.arange(n, dtype=np.int64) * 3 + 5
    for seed, node, fragment, count in ((0, 0, 0, n), (0x9E3779B97F4A7C15, 4095, 63, 64), (7, 17, 5, 64)):
        got = analysis.debris_directions(seed, ids[:count], node, fragment)
        want = np.array([debris_ref.direction(seed, int(i), node, fragment) for i in ids[:count]]).T
        assert got.shape == (3, count) and np.array_equal(got, want), (seed, node, fragment)
        if count == n:
            assert (np.abs(got.mean(axis=1)) <= 4.0 / math.sqrt(3.0 * n)).all(), got.mean(axis=1)
            length = np.sqrt((got[0] * got[0] + got[1] * got[1]) + got[2] * got[2])
            assert (np.abs(length - 1.0) <= 4.0 * 2.0 ** -52).all()
    # ids beyond 2^32 reach counter word 1; a window equals the whole; the hook reaches the fallback
    big = np.array([(1 << 40) + 3, (1 << 32), (1 << 32) - 1], dtype=np.int64)
    got = analysis.debris_directions(11, big, 3, 2)
    assert np.array_equal(got, np.array([debris_ref.direction(11, int(i), 3, 2) for i in big]).T)
    assert np.array_equal(analysis.debris_directions(0, ids[100:200], 0, 0), analysis.debris_directions(0, ids, 0, 0)[:, 100:200])
    assert debris_ref.direction(0, 0, 0, 0, pairs=lambda t: (0.9, -0.9)) == (0.0, 0.0, 1.0)
    for bad in (dict(node=-1), dict(node=4096), dict(fragment=64), dict(fragment=-1)):
        kw = dict(node=0, fragment=0)
        kw.update(bad)
        with pytest.raises(_abi.ErplError):
            analysis.debris_directions(0, ids[:2], **kw)


def test_step_rule_and_ticks():
    assert debris_ref.halvings(1.0, 0.25, 0.25) == (0, 1.0) and debris_ref.halvings(np.nextafter(1.0, 2.0), 0.25, 0.25) == (1, 0.5)
    assert debris_ref.halvings(128.0, 0.25, 0.25) == (7, 2.0 ** -7) and debris_ref.halvings(1e30, 0.25, 0.25) == (16, 2.0 ** -16)
    assert debris_ref.halvings(float("nan"), 0.25, 0.25) == (16, 2.0 ** -16) and debris_ref.halvings(0.0, 0.25, 1.0) == (0, 1.0)
    for n, wq, dt in ((0, 0.3, 0.05), (17, 0.9999999999999999, 0.1), (19999, 0.5, 1.0 / 3.0)):
        assert debris_ref.tfall(n << 16, wq, 0, dt) == (float(n) + wq) * dt
    assert debris_ref.tfall(3 * 65536 + 2 * 32768, 0.5, 2, 0.25) == 4.125 * 0.25


def test_summary_rows():
    sq = [(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0)]
    # five records 1 s apart, stride 1, three fragments; row k * 3 + f
    rec = np.zeros((5, 15))
    rec[:, 0] = 0.25 + np.arange(5)
    rec[:, 7] = 1.0
    nan = np.nan
    #        node 0           node 1 (none lands)   node 2            node 3            node 4
    X = [1.0, 2.0, nan,      nan, nan, nan,         3.0, 7.0, 7.0,    7.0, 1.0, -2.0,   1.0, nan, nan]
    Y = [1.0, 1.0, nan,      nan, nan, nan,         1.0, 0.5, 0.5,    0.5, 9.0, 1.0,    1.0, nan, nan]
    T = [5.0, 9.0, nan,      nan, nan, nan,         9.0, 2.0, 2.0,    1.0, 9.0, 3.0,    1.0, nan, nan]
    vals = np.full((5, 18), nan)                                # a sixth node that is never evaluated
    for i, (x, y, t) in enumerate(zip(X, Y, T)):
        if np.isfinite(x):
            vals[:, i] = (x, y, math.hypot(x, y), t, 2.0)
    row, pick = debris_ref.summary_of(vals, rec, 1, 3, keep_in=sq)
    assert row[A.DEBRIS_NODES] == 5 and row[A.DEBRIS_LANDED] == 9
    # the farthest: (1, 9) of job 10 beats the three (7, 0.5); among those alone job 7 would win the tie
    assert pick["far"] == 10 and row[A.DEBRIS_MAX_RANGE] == math.hypot(1.0, 9.0) and row[A.DEBRIS_MAX_RANGE_TIME] == 3.0
    assert row[A.DEBRIS_MAX_RANGE_X] == 1.0 and row[A.DEBRIS_MAX_RANGE_Y] == 9.0 and row[A.DEBRIS_MAX_RANGE_FRAGMENT] == 1
    # the longest fall: 9 s three times, the lowest index wins
    assert pick["slow"] == 1 and row[A.DEBRIS_MAX_TFALL] == 9.0 and row[A.DEBRIS_MAX_TFALL_TIME] == 0.0
    # outside the square: jobs 7, 8 (x = 7), 9 (x = 7), 10 (y = 9), 11 (x = -2): node 2 is the first, fragment 1 the lowest there
    assert row[A.DEBRIS_OUTSIDE] == 5 and pick["exit"] == 7 and row[A.DEBRIS_EXIT_TIME] == 2.0 and row[A.DEBRIS_EXIT_FRAGMENT] == 1
    assert row[A.DEBRIS_EXIT_X] == 7.0 and row[A.DEBRIS_EXIT_Y] == 0.5
    # the bounding boxes: node 0: 1 x 0, node 2: 4 x 0.5, node 3: 9 x 8.5, node 4: a point
    assert pick["wide"] == 3 and row[A.DEBRIS_MAX_SPREAD] == math.sqrt(9.0 * 9.0 + 8.5 * 8.5) and row[A.DEBRIS_MAX_SPREAD_TIME] == 3.0
    far_only = vals.copy()
    far_only[:, 10] = nan
    row, pick = debris_ref.summary_of(far_only, rec, 1, 3, keep_in=sq)
    assert pick["far"] == 7 and row[A.DEBRIS_MAX_RANGE_FRAGMENT] == 1 and row[A.DEBRIS_LANDED] == 8 and row[A.DEBRIS_OUTSIDE] == 4
    # no polygon: the exit rows and OUTSIDE are NaN; a polygon that holds everything: OUTSIDE = 0, no exit
    row, pick = debris_ref.summary_of(vals, rec, 1, 3)
    assert np.isnan(row[A.DEBRIS_EXIT_TIME:A.DEBRIS_EXIT_Y + 1]).all() and np.isnan(row[A.DEBRIS_OUTSIDE]) and pick["exit"] == -1
    row, pick = debris_ref.summary_of(vals, rec, 1, 3, keep_in=[(-50.0, -50.0), (50.0, -50.0), (50.0, 50.0), (-50.0, 50.0)])
    assert row[A.DEBRIS_OUTSIDE] == 0 and np.isnan(row[A.DEBRIS_EXIT_TIME]) and pick["exit"] == -1
    # a single landed job per node: spread 0 at the first such node; the usable prefix ends at record 3: nodes 0..1 at stride 2
    rec[3, 9] = nan
    two = np.full((5, 6), nan)
    two[:, 0] = (1.0, 1.0, math.hypot(1.0, 1.0), 5.0, 2.0)
    two[:, 5] = (3.0, 1.0, math.hypot(3.0, 1.0), 5.0, 2.0)
    row, pick = debris_ref.summary_of(two, rec, 2, 3)
    assert row[A.DEBRIS_NODES] == 2 and row[A.DEBRIS_LANDED] == 2 and pick["wide"] == 0 and row[A.DEBRIS_MAX_SPREAD] == 0.0
    assert pick["slow"] == 0 and pick["far"] == 5 and row[A.DEBRIS_MAX_RANGE_TIME] == 2.0
    rec[0, 3] = nan
    row, pick = debris_ref.summary_of(two, rec, 2, 3, keep_in=sq)
    assert row[A.DEBRIS_NODES] == 0 and row[A.DEBRIS_LANDED] == 0 and row[A.DEBRIS_OUTSIDE] == 0 and np.isnan(row[:13]).all()
