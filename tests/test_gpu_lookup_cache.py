"""The cached table lookups of erpl_k_lookup.h ON THE DEVICE: WindCache, MachCache, AtmCache and (fp64 throughput build)
the lane's wind record in LDS live across RHS evaluations, but erpl_mc_debug_eval(ERPL_DBG_RHS) starts every lane with
empty caches.  ERPL_DBG_RHS_SEQ runs one lane per sample through a whole sequence of states with ONE set of caches, and
the latch comes from each column's input, so its results must be those of the stateless evaluation BIT FOR BIT: a cache
hit, the neighbour guess of mach_reload, the straight-line guess of wind_reload against its bisection, a wind-knot crossing
inside one atmosphere layer, the read-modify-write of the LDS wind record, the recovery after a NaN altitude or Mach
number.  No tolerance: a stale interval reused one evaluation past a knot, a lane that reads its neighbour's LDS slot or
an off-by-one at h == knot all change bits.  The columns at and next to a knot and behind each NaN are compared with the
CPU oracle too, on the lane's own sample, so that the fresh evaluation is itself pinned where the tables switch records.

96 dispersed samples (one full wave and half of one, every lane its own wind table), 256 states per lane, each lane with
its own phase and stride through a tour of altitudes and a tour of Mach numbers (tour_* below)."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, flatten, models

import helpers as H
from math_inputs import DTYPES, cast
from test_gpu_kat import TOL, block_err

N_LANES, N_STATES = 96, 256
NAN_ALT_AT, NAN_VEL_AT = 128, 160          # the state of every lane with a NaN altitude / a NaN velocity
LAYER_EDGES = (11000.0, 20000.0, 25000.0, 32000.0)
GAMMA_R = 1.4 * 287.053
GRIDS = ["csv", "uniform100", "random37", "k2", "max_knots", "no_wind"]


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def wind_grid(name):
    """(altitude knots, base wind [K, 3]) of a grid, or (None, None): the 100-knot synthetic profile / no table."""
    rs = np.random.RandomState(3)
    if name == "csv":
        return H.CSV_ALT, H.CSV_WIND
    if name in ("uniform100", "no_wind"):
        return None, None
    if name == "random37":   # strictly increasing, gaps of 1/8 m .. 9.5 km (values fp32 holds exactly): the straight line misses
        alt = np.cumsum(np.round(10.0 ** rs.uniform(-0.9, 4.1, 37) * 8.0) / 8.0) - 300.0
        assert np.all(np.diff(alt) > 0) and alt[-1] > 32000.0
    elif name == "k2":
        alt = np.array([1000.0, 18000.0])
    else:
        alt = np.arange(_abi.MAX_WIND_KNOTS) * 40.0
    wind = np.stack([rs.normal(8.0, 6.0, alt.size), rs.normal(0.0, 4.0, alt.size), rs.normal(0.0, 0.5, alt.size)], axis=1)
    return alt, wind


_BATCHES = {}


def host_batch(kind, grid):
    if (kind, grid) not in _BATCHES:
        alt, wind = wind_grid(grid)
        params = flatten.generate_parameter_samples(H.UNCERTAINTY, N_LANES)
        hb = flatten.dispersed_batch(models.Rocket(), H.make_motor(kind), models.WindModel(), H.EXAMPLE_IC, params, alt, wind)
        if grid == "no_wind":
            nb = flatten.HostBatch(N_LANES, 0)
            nb.ic, nb.rocket, nb.motor = hb.ic, hb.rocket, hb.motor
            hb = nb
        assert hb.n == N_LANES and hb.k_wind == {"csv": 6, "uniform100": 100, "random37": 37, "k2": 2,
                                                 "max_knots": _abi.MAX_WIND_KNOTS, "no_wind": 0}[grid]
        _BATCHES[kind, grid] = hb
    return _BATCHES[kind, grid]


def three_around(v, dtype):
    v = dtype(v)
    return [float(np.nextafter(v, dtype(-np.inf))), float(v), float(np.nextafter(v, dtype(np.inf)))]


def tour_altitudes(knots, dtype):
    """One trip up and down again (values of `dtype`, flag = at or next to a knot or layer edge): below the first knot;
    every wind knot and every layer edge as the float just below it, the value itself and the float just above it; three
    consecutive points inside every interval; above the last knot and the last edge; +1e31 (the kBig clamp); then the same
    downwards to -1e31.  With more than 100 knots only every 16th knot gets its two neighbours and every interval one point."""
    knots = cast(knots, dtype)
    dense = len(knots) <= 100
    marks = sorted(set(knots.tolist()) | set(LAYER_EDGES))
    up, flag = [min(marks[0], 0.0) - 250.0, marks[0] - 3.0], [False, False]
    for i, v in enumerate(marks):
        full = dense or i % 16 == 0 or v in LAYER_EDGES
        pts = three_around(v, dtype) if full else [v]
        up += pts
        flag += [True] * len(pts)
        nxt = marks[i + 1] if i + 1 < len(marks) else v + 9000.0
        inside = [v + f * (nxt - v) for f in ((0.3, 0.5, 0.7) if dense else (0.5,))]
        up += inside
        flag += [False] * len(inside)
    up += [60000.0, 1e31]
    flag += [False, False]
    alt = np.array(up + up[::-1] + [-50.0, -1e31], dtype=np.float64)
    return cast(alt, dtype), np.array(flag + flag[::-1] + [False, False])


def tour_mach(union, dtype):
    """(Mach number, ulps the speed is moved by, flag) up and down: for every union knot of the Cd and CP-shift tables 0.1 %
    below it, the speed that lands on it moved by -2 .. 2 ulps (on the knot exactly in the gate's arithmetic where the wind is
    zero; within a few ulps of it elsewhere), 0.1 % above it, then two points inside the interval; slow (Mach 1e-5) and past
    the last knot at both ends."""
    up = [(1e-5, 0, False), (0.02, 0, False)]
    for i, u in enumerate(union):
        if u > 0:
            up.append((u * 0.999, 0, True))
            up += [(u, k, True) for k in (-2, -1, 0, 1, 2)]
            up.append((u * 1.001, 0, True))
        nxt = union[i + 1] if i + 1 < len(union) else u + 1.5
        up += [(u + 0.35 * (nxt - u), 0, False), (u + 0.7 * (nxt - u), 0, False)]
    up.append((6.0, 0, False))
    t = up + up[::-1]
    return np.array([a for a, _, _ in t]), np.array([k for _, k, _ in t]), np.array([f for _, _, f in t])


def isa_temperature(h):
    """Temperature of environment.py:26-103 (for choosing speeds only; the oracle is the reference)."""
    h = np.nan_to_num(np.asarray(h, dtype=np.float64), nan=0.0)
    t = np.where(h <= 11000.0, 288.15 - 0.0065 * np.clip(h, -1e5, 11000.0),
                 np.where(h <= 20000.0, 216.65, np.where(h <= 32000.0, np.minimum(216.65 + 0.001 * (h - 20000.0), 228.65),
                                                         np.maximum(228.65 - 0.0028 * (np.minimum(h, 1e6) - 32000.0), 180.0))))
    return np.maximum(t, 150.0)


def build_states(hb, kind, dtype):
    """x [16, N_STATES * N_LANES]: column i * N_LANES + lane is state i of that lane (the order ERPL_DBG_RHS_SEQ walks in);
    near [same]: columns whose altitude or Mach number is at or next to a knot, or that follow a NaN, at altitudes
    within +-100 km."""
    cfg = H.make_config(kind)
    union = sorted(set(list(cfg.cd_mach)[:cfg.n_cd]) | set(list(cfg.cp_mach)[:cfg.n_cp]))
    alt_t, alt_f = tour_altitudes(hb.alt_grid if hb.k_wind else np.array([0.0, 5000.0, 15000.0]), dtype)
    mach_t, mach_k, mach_f = tour_mach(cast(union, dtype).tolist(), dtype)
    rs = np.random.RandomState(23)
    n, m = N_LANES, N_STATES * N_LANES
    lane = np.arange(n)
    i = np.arange(N_STATES)[:, None]
    # every lane its own phase; three of four lanes walk the altitude tour point by point, the others skip one to two and two
    # to four knots per step; two of three lanes walk the Mach tour point by point, the others jump across knots
    a_stride = np.where(lane % 4 == 3, 7, np.where(lane % 4 == 2, 13, 1))
    m_stride = np.where(lane % 3 == 0, 5, 1)
    ai = ((lane * len(alt_t)) // n + i * a_stride) % len(alt_t)          # [N_STATES, n]
    mi = ((lane * 11) % len(mach_t) + i * m_stride) % len(mach_t)
    h, near = alt_t[ai], alt_f[ai] | mach_f[mi]
    h[NAN_ALT_AT] = np.nan
    speed = mach_t[mi] * np.sqrt(GAMMA_R * isa_temperature(h))
    for k in (-2, -1, 1, 2):
        mv = mach_k[mi] == k
        for _ in range(abs(k)):
            speed[mv] = np.nextafter(speed[mv], np.inf if k > 0 else -np.inf)
    wind = np.zeros((3,) + h.shape)
    if hb.k_wind:
        for l in range(n):
            hq = np.nan_to_num(np.clip(h[:, l], -1e30, 1e30), nan=0.0)
            for c in range(3):
                wind[c, :, l] = np.interp(hq, hb.alt_grid, hb.wind[:, c, l])
    x = np.zeros((16, N_STATES, n))
    x[0] = np.where(i % 5 == 4, 40.0, rs.uniform(0.1, 14.9, (N_STATES, n)))        # burning, every fifth state burnt out
    x[1:3] = rs.normal(0.0, 500.0, (2, N_STATES, n))
    x[3] = h
    # velocity along the body axis (identity attitude: body x is inertial x) and ~1 % across it, in still air; the wind on top
    x[4] = wind[0] + speed
    x[5] = wind[1] + speed * rs.normal(0.0, 0.01, (N_STATES, n))
    x[6] = wind[2] + speed * rs.normal(0.0, 0.01, (N_STATES, n))
    x[4, NAN_VEL_AT] = np.nan
    x[7] = 1.0
    x[11:14] = rs.normal(0.0, 0.2, (3, N_STATES, n))
    x[14] = np.where(i % 5 == 4, 0.0, rs.uniform(0.05, 1.0, (N_STATES, n)))
    x[15] = rs.rand(N_STATES, n) < 0.05
    near[NAN_ALT_AT + 1] = True
    near[NAN_VEL_AT + 1] = True
    near[NAN_ALT_AT] = near[NAN_VEL_AT] = False
    with np.errstate(invalid="ignore"):
        near &= np.abs(h) <= 1e5     # (at +-1e31 m the Mach number means nothing, and fp32 overflows where fp64 does not)
    return cast(x.reshape(16, m), dtype) if dtype == np.float32 else x.reshape(16, m), near.reshape(m), (ai, mi, union)


def klass(a):
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def test_sequences_cover_what_they_claim():
    """(No device work.)  Every interval of every wind grid and of the Mach table is visited, every knot and layer edge is hit
    exactly and from both neighbouring floats, lanes of one wave are in different intervals at the same step, there are runs
    inside one interval, single-knot crossings and steps across two and more knots."""
    for dtype in (np.float64, np.float32):
        for grid in GRIDS:
            hb = host_batch("liquid", grid)
            x, near, (ai, mi, union) = build_states(hb, "liquid", dtype)
            h = x[3].reshape(N_STATES, N_LANES)
            assert np.isnan(h[NAN_ALT_AT]).all() and np.isnan(x[4].reshape(N_STATES, N_LANES)[NAN_VEL_AT]).all()
            assert np.isnan(x).sum() == 2 * N_LANES
            assert (h == 1e31).any() or dtype == np.float32 and (h == float(np.float32(1e31))).any()
            assert (h < -1e30).any() and near.sum() >= 2000
            for e in LAYER_EDGES:
                assert all((h == v).any() for v in three_around(e, dtype)), (grid, e)
            if hb.k_wind:
                knots = cast(hb.alt_grid, dtype)
                ok = np.isfinite(h)
                idx = np.where(ok, np.searchsorted(knots, np.where(ok, h, 0.0), side="right"), -1)
                assert set(range(hb.k_wind + 1)) <= set(idx.ravel().tolist()), grid
                assert np.isin(knots, h).all(), grid
                if hb.k_wind <= 100:
                    assert np.isin(np.nextafter(knots.astype(dtype), dtype(-np.inf)).astype(np.float64), h).all()
                    assert np.isin(np.nextafter(knots.astype(dtype), dtype(np.inf)).astype(np.float64), h).all()
                step = np.abs(np.diff(idx, axis=0))[(idx[1:] >= 0) & (idx[:-1] >= 0)]
                assert (step == 0).sum() >= 1000 and (step == 1).sum() >= 1000 and ((step >= 2).sum() >= 1000 or hb.k_wind == 2)
                assert min(len(set(idx[s, :64].tolist())) for s in (1, 50, 200)) >= (3 if hb.k_wind > 2 else 2)
            assert set(range(mi.max() + 1)) <= set(mi.ravel().tolist()) and len(union) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("kind", ["liquid", "solid"])
@pytest.mark.parametrize("precision", ["f64", "f64_fast", "f32"])
def test_cached_evaluation_is_the_fresh_one(engine, oracle, precision, kind, grid):
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    dtype = DTYPES[precision]
    hb = host_batch(kind, grid)
    cfg = H.make_config(kind)
    engine.set_config(cfg)
    db = DeviceBatch.from_host(hb, engine.device, _abi.PRECISIONS[precision])
    x, near, _ = build_states(hb, kind, dtype)
    fresh = engine.debug_eval(db, _abi.DBG_RHS, x)
    seq = engine.debug_eval(db, _abi.DBG_RHS_SEQ, x)
    same = (fresh == seq) | (np.isnan(fresh) & np.isnan(seq))
    bad = np.argwhere(~same)
    if len(bad):
        r, c = bad[0]
        print(f"{precision}/{kind}/{grid}: {len(set(bad[:, 1].tolist()))} columns differ, first: row {r}, state {c // N_LANES} of "
              f"lane {c % N_LANES}, h = {x[3, c]!r}: cached {seq[r, c]!r}, fresh {fresh[r, c]!r}")
    assert same.all()
    assert np.isnan(fresh[3:6]).any() and np.isfinite(fresh[:14]).all(axis=0).sum() > 0.9 * x.shape[1]

    # the fresh evaluation against the oracle where the tables switch records and behind each NaN: at most 2000 columns,
    # the same number from every lane
    per_lane = 2000 // N_LANES
    cols = []
    for l in range(N_LANES):
        c = np.flatnonzero(near.reshape(N_STATES, N_LANES)[:, l])
        must = [s for s in (NAN_ALT_AT + 1, NAN_VEL_AT + 1) if s in c]
        rest = [s for s in c[np.linspace(0, len(c) - 1, per_lane).astype(int)] if s not in must][:per_lane - len(must)]
        cols += [s * N_LANES + l for s in must + rest]
    assert N_LANES * 10 <= len(cols) <= 2000
    lanes = {l: hb.take([l]) for l in range(N_LANES)}
    exp = np.zeros((15, len(cols)))
    for k, c in enumerate(cols):
        d, chute = oracle.rhs(cfg, lanes[c % N_LANES], x[0, c], x[1:15, c], int(x[15, c]))
        exp[:14, k], exp[14, k] = d, chute
    got = fresh[:, cols]
    assert np.array_equal(got[14], exp[14])
    if precision == "f64":
        assert np.array_equal(klass(got[:14]), klass(exp[:14]))
    assert np.isfinite(exp[:14]).all()
    err = block_err(got[:14], exp[:14])
    print(f"{precision}/{kind}/{grid}: cached == fresh over {x.shape[1]} columns; fresh vs oracle at {len(cols)} knot / "
          f"after-NaN columns: worst block error {err:.2e}")
    assert err < TOL[precision]["rhs"]


def late_start_motor():
    """The solid motor without the first knot of its thrust curve: the curve starts at 0.2 s, so that `before the first
    knot` exists at times the RHS is called with (t >= 0)."""
    m = H.make_motor("solid")
    m.thrust_curve_time = m.thrust_curve_time[1:]
    m.thrust_curve_normalized = m.thrust_curve_normalized[1:]
    m.thrust_curve_thrust = m.thrust_curve_thrust[1:]
    return m


def rhs_at_times(engine, oracle, precision, cfg, hb, t):
    """The RHS of one climbing, burning state at the times t: (device [15, m], oracle [15, m])."""
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    t = np.asarray(t, dtype=np.float64)
    x = np.zeros((16, t.size))
    x[0] = t
    x[3] = 1500.0
    x[4], x[5], x[6] = 180.0, 3.0, 120.0
    x[7:11] = np.array([0.7933533, 0.0, -0.6087614, 0.0])[:, None]      # pitched 75 degrees up
    x[12] = 0.05
    x[14] = 0.6
    engine.set_config(cfg)
    got = engine.debug_eval(DeviceBatch.from_host(hb, engine.device, _abi.PRECISIONS[precision]), _abi.DBG_RHS, x)
    exp = np.array([np.append(*oracle.rhs(cfg, hb, x[0, j], x[1:15, j], 0)) for j in range(t.size)]).T
    return got, exp


def longest_burning_lane(kind):
    hb = host_batch(kind, "csv")
    return hb.take([int(np.argmax(hb.motor[3]))])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f64", "f64_fast", "f32"])
def test_rhs_on_thrust_curve_knots(engine, oracle, precision):
    """Stateless side: t on every thrust-curve knot of the solid motor and one ulp either side of it, after the last knot
    (a sample that still burns there), before the first knot (the curve that starts at 0.2 s), t == burn_time, one ulp
    before and one ulp past it (both motors) - against the oracle at the tolerance of the RHS vectors.  Times below zero:
    test_rhs_before_time_zero."""
    up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    for kind, motor in (("solid", None), ("solid", late_start_motor()), ("liquid", None)):
        cfg = H.make_config(kind) if motor is None else flatten.config_from_objects(models.Rocket(), motor, models.StandardAtmosphere())
        hb = longest_burning_lane(kind)
        burn = float(hb.motor[3, 0])
        t = [down(burn), burn, up(burn), 0.0, 1e-9, burn + 7.0]
        if kind == "solid":
            knots = list(cfg.curve_time)[:cfg.n_curve]
            assert len(knots) == (10 if motor is None else 9) and burn > knots[-1] + 0.01
            for v in knots:
                t += [down(v), v, up(v)] if v > 0 else [v, up(v)]
            t += [0.5 * (knots[-1] + burn)]                     # after the last knot, still burning
            if motor is not None:
                t += [0.1, 0.19]                                # before the first knot
        got, exp = rhs_at_times(engine, oracle, precision, cfg, hb, t)
        assert np.array_equal(got[14], exp[14])
        assert (exp[13] == 0).sum() == 2 and (exp[13] < 0).sum() == len(t) - 2        # the burn gate closes right behind burn_time
        err = block_err(got[:14], exp[:14])
        print(f"{precision}/{kind}: RHS at {len(t)} thrust-curve / burn-time knots, worst block error {err:.2e}")
        assert err < TOL[precision]["rhs"]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f64", "f64_fast", "f32"])
def test_rhs_before_time_zero(engine, oracle, precision):
    """`Before the first knot` of the solid motor's curve as shipped (first knot at t = 0) means t < 0: one ulp below zero,
    -0.5 s and -1 s, both motors, against the oracle at the tolerance of the RHS vectors.  motor.py gates thrust and mass
    flow with `time < 0 or time > burn_time`; the kernels' burn gate used to be `pf > 0 and t <= burn_time` alone, so that
    below zero the device burnt (propellant rate -mdot / prop against the reference's 0: block error 5.5e10 in all three
    builds; axial acceleration 4.11 against 3.80 m/s^2 with the solid motor).  No flight reaches t < 0 - the integration
    starts at the rail-exit time >= 0 - so no summary moved when `t >= 0` joined the gate."""
    for kind in ("solid", "liquid"):
        got, exp = rhs_at_times(engine, oracle, precision, H.make_config(kind), longest_burning_lane(kind), [-5e-324, -0.5, -1.0])
        err = block_err(got[:14], exp[:14])
        print(f"{precision}/{kind}: RHS at t < 0: worst block error {err:.2e}; pf rate device {got[13].tolist()}, "
              f"oracle {exp[13].tolist()}; axial acceleration device {got[3].tolist()}, oracle {exp[3].tolist()}")
        assert np.array_equal(got[14], exp[14]) and (exp[13] == 0).all()
        assert err < TOL[precision]["rhs"]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f64", "f64_fast", "f32"])
def test_aero_on_mach_knots(engine, oracle, precision):
    """Stateless side: Mach on every union knot of the Cd and CP-shift tables (as the build holds it) and on the floats next to
    it, power on and off, against the oracle at the tolerance of the aero vectors."""
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    dtype = DTYPES[precision]
    cfg = H.make_config("liquid")
    engine.set_config(cfg)
    hb = host_batch("liquid", "csv").take([9])
    union = sorted(set(list(cfg.cd_mach)[:cfg.n_cd]) | set(list(cfg.cp_mach)[:cfg.n_cp]))
    mach = np.array([v for u in cast(union, dtype) for v in three_around(u, dtype) if v >= 0] + [4.0, 7.5])
    rows = np.array([[m, a, b, pf, float(pf > 0)] for m in mach for a, b in ((0.03, -0.02), (-0.2, 0.1), (0.4, 0.0))
                     for pf in (0.7, 0.0)])
    db = DeviceBatch.from_host(hb, engine.device, _abi.PRECISIONS[precision])
    got = engine.debug_eval(db, _abi.DBG_AERO, rows.T)
    exp = np.array([oracle.aero(cfg, r[0], r[1], r[2], oracle.mass_props(cfg, hb.rocket[0, 0], hb.rocket[1, 0], r[3])[1],
                                r[4] > 0)[:5] for r in rows]).T
    err = np.abs(got - exp) / np.maximum(np.abs(exp), 0.1)
    print(f"{precision}: aero on {mach.size} Mach knots and neighbours x 6: worst err {err.max():.2e}")
    assert len(union) == 8 and err.max() < TOL[precision]["aero"]
