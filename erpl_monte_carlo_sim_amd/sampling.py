"""Vectorised dispersion + wind-profile synthesis in torch.

The reference draws every sample from a legacy MT19937 `RandomState(i)` in Python loops
(monte_carlo.py:156-179, environment.py:125-265), ~ms per sample.  `flatten.dispersed_batch`
restates that bit for bit and is what the parity sets use.  For the 100 k - 10 M throughput
configurations this module draws the SAME distributions with torch's counter-based generator,
all samples at once, directly into the SoA tensors the kernels read (no host round trip), with the AR(1)
wind recursion in one HIP kernel of the C ABI (erpl_mc_synth_wind).  It is not bit-identical to MT19937
and is therefore never used for parity against the reference; its distribution is tested against the
bit-exact host generator (tests/test_gpu_sampling.py).
"""
import math

import torch

from . import _abi
from .engine import DeviceBatch
from .flatten import motor_kind, reject_overrides
from .models import knot_constants

DEFAULT_UNCERTAINTY = {
    "initial_position": [0.0, 0.0, 0.0],
    "initial_velocity": [0.1, 0.1, 0.1],
    "initial_attitude": [0.005, 0.005, 0.005],
    "initial_angular_velocity": [0.005, 0.005, 0.005],
    "mass_uncertainty": 0.02,
    "thrust_uncertainty": 0.03,
    "wind_speed_range": [0.0, 5.0],
    "wind_direction_range": [0.0, 2 * math.pi],
    "atmospheric_density_uncertainty": 0.05,
}


# rows of DeviceBatch.factors, in order (the liquid motor's mass-flow multiplier is absent for a solid motor)
FACTOR_NAMES = ("position_x", "position_y", "position_z", "velocity_x", "velocity_y", "velocity_z",
                "attitude_roll", "attitude_pitch", "attitude_yaw",
                "angular_velocity_x", "angular_velocity_y", "angular_velocity_z",
                "mass_multiplier", "motor_thrust_multiplier", "motor_mass_flow_multiplier",
                "wind_speed", "wind_direction", "wind_mean_u", "wind_mean_v")


def _euler_to_quaternion(roll, pitch, yaw):
    cr, sr = torch.cos(roll / 2), torch.sin(roll / 2)
    cp, sp = torch.cos(pitch / 2), torch.sin(pitch / 2)
    cy, sy = torch.cos(yaw / 2), torch.sin(yaw / 2)
    return torch.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                        cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


def _check_ranges(ic, rk, mt, mean_u, mean_v):
    """The input contract `DeviceBatch.from_host` enforces, for batches generated on the device: the
    kernels assume finite inputs, positive masses and mass flow, a finite non-negative burn time.  (The
    wind table is a finite linear map of the finite normals, per-knot constants and mean-wind rows.)"""
    ok = (torch.isfinite(ic).all() & torch.isfinite(rk).all() & torch.isfinite(mt).all()
          & torch.isfinite(mean_u).all() & torch.isfinite(mean_v).all()
          & (rk > 0).all() & (mt[2] > 0).all() & (mt[3] >= 0).all())
    if not bool(ok):
        raise _abi.ErplError("generated dispersions violate the kernel input contract (finite values, positive "
                             "masses and mass flow): check the uncertainty table")


def primitive_rows(K):
    """Rows of the primitive tensor of the independent law for K wind knots: 14 dispersion normals, 3 motor normals, 3 K
    turbulence normals, 2 uniforms."""
    return 17 + 3 * int(K) + 2


def primitive_draws(n, K, device, seed):
    """The float64 [17 + 3 K + 2, n] primitives of the independent law (`synthetic_dispersions(draws=...)`) on `device`,
    from torch's counter-based generator at `seed`: normals, and in the last two rows uniforms in [0, 1)."""
    device = torch.device(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    z = torch.randn((17 + 3 * int(K), int(n)), generator=gen, dtype=torch.float64, device=device)
    uni = torch.rand((2, int(n)), generator=gen, dtype=torch.float64, device=device)
    return torch.cat([z, uni]).contiguous()


def design_draws(n, K, device, seed, design="lhs", block=0, first=0, count=None, engine=None):
    """Columns first .. first + count - 1 (default: all from `first`) of the float64 [17 + 3 K + 2, n] primitives of the
    independent law as ONE design of n columns (erpl_mc_design): the row kinds of `primitive_draws`, normals and in the last
    two rows uniforms - here in (0, 1), which every consumer of the [0, 1) rows accepts.  design: 'random' (independent
    draws), 'lhs' (every row stratified: each of the m strata of a replicate holds one column) or 'lhs_centred'; block = m:
    n / m independent replicates of m columns each, 0 = n.  Counter-based on (seed, row, column): a window is the same bits
    whatever rank or sub-batch generates it.  design 'qmc' (erpl_mc_qmc): a scrambled Sobol' design on the dimensions of
    `qmc_dims(K)`, the rows without a dimension padded with independent draws; its replicates are independently scrambled
    nets, and with block = 0 no column depends on n, so the columns [n, 2 n) of a design of 2 n continue a design of n."""
    device = torch.device(device)
    if engine is None:
        from .simulator import shared_engine
        engine = shared_engine(device)
    kinds = [_abi.DESIGN_NORMAL] * (17 + 3 * int(K)) + [_abi.DESIGN_UNIFORM] * 2
    if design == "qmc":
        return engine.qmc(kinds, n, seed, dims=qmc_dims(K), scramble="owen", pad="random", block=block, first=first, count=count)
    return engine.design(kinds, n, seed, kind=design, block=block, first=first, count=count)


def qmc_dims(K, liquid=True):
    """The Sobol' dimension of every row of the primitive tensor for `design_draws(design='qmc')`, -1 for a pad row.  The
    low dimensions of a Sobol' sequence are its best, so the scalar primitives of `scalar_primitives` take them, in its
    order - wind speed and direction, the last two ROWS, among them - then the 3 K turbulence innovations in row order as
    far as the 1024 dimensions of erpl_mc_qmc go.  What is left of those, and the dead draws, are pad rows."""
    K = int(K)
    dims = [-1] * primitive_rows(K)
    order = list(scalar_primitives(K, liquid).values()) + list(range(17, 17 + 3 * K))
    for d, r in enumerate(order[:_abi.QMC_MAX_DIMS]):
        dims[r] = d
    return dims


def primitive_groups(K, liquid=True):
    """The default factors of a pick-freeze design: an ordered mapping group name -> rows of the primitive tensor.  Rows 16
    (and 15 for a solid motor: its burn-time and impulse draws, drawn then unused) belong to no group."""
    K = int(K)
    groups = {"position": [0, 1, 2], "velocity": [3, 4, 5], "attitude": [6, 7, 8], "angular_velocity": [9, 10, 11],
              "mass": [12], "dead_draw": [13], "motor_thrust": [14]}
    if liquid:
        groups["motor_mass_flow"] = [15]
    groups["wind_speed"] = [17 + 3 * K]
    groups["wind_direction"] = [17 + 3 * K + 1]
    groups["turbulence"] = list(range(17, 17 + 3 * K))
    return groups


def scalar_primitives(K, liquid=True):
    """The default variables of a polynomial chaos surrogate: an ordered mapping name -> row of the primitive tensor for the
    scalar primitives of `primitive_groups` - every group but the 3 K turbulence innovations and the dead draw - a
    three-row group as name_x, name_y, name_z."""
    out = {}
    for name, rows in primitive_groups(K, liquid).items():
        if name in ("turbulence", "dead_draw"):
            continue
        for i, r in enumerate(rows):
            out[name if len(rows) == 1 else f"{name}_{'xyz'[i]}"] = r
    return out


_SIGMA_ROWS = {"initial_position": (0, 1, 2), "initial_velocity": (3, 4, 5), "initial_attitude": (6, 7, 8),
               "initial_angular_velocity": (9, 10, 11)}
_PLANAR_ZEROED = (4, 6, 8, 9, 11)    # velocity y, roll, yaw, angular velocity x and z: Set P multiplies them by zero


def law_change(K, liquid, flown, target, motor=None, target_motor=None, shift=None, planar=False):
    """The primitives whose law differs between two uncertainty tables of `synthetic_dispersions(draws=...)`, as erpl_mc_reweight
    takes them: an ordered mapping primitive row -> (kind, mu, s, a, b), ascending in the row, at most 32.

    flown, target: uncertainty tables (None or partial: DEFAULT_UNCERTAINTY, then `flown`, then `target` on top).  The sigma
    entries initial_position, initial_velocity, initial_attitude and initial_angular_velocity are per component and, like
    mass_uncertainty (row 12), give a normal row with s = target / flown: the flown value is base + sigma z, so under the
    target z ~ N(0, s^2) in flown sigmas.  wind_speed_range and wind_direction_range (the last two rows) give a uniform
    row with (a, b) = the target range within the flown one.  The motor's thrust_uncertainty (row 14) and, for a liquid
    motor, mass_flow_uncertainty (row 15) are read from `motor` (flown) and `target_motor`.  shift: a mapping
    `scalar_primitives` name (or the row of a normal primitive) -> mu, the target mean in flown sigmas.
    planar=True leaves out the rows Set P zeroes: they reach no outcome, and weighting them only adds noise.

    ValueError: a flown sigma of 0 with another target (nothing was varied: there is nothing to reweight); a target sigma of
    0 (a point law has no density ratio); a target range that is not inside the flown one (a weight cannot create samples);
    a key without a primitive - thrust_uncertainty of the table (the reference's dead draw: the motor's own entry is the
    live one) and atmospheric_density_uncertainty; more than 32 changed rows."""
    K, liquid = int(K), bool(liquid)
    base = {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in DEFAULT_UNCERTAINTY.items()}
    for table in (flown, target):
        for key in (table or {}):
            if key not in DEFAULT_UNCERTAINTY:
                raise ValueError(f"{key!r} is no entry of the uncertainty table")
    base.update(flown or {})
    new = dict(base)
    new.update(target or {})
    first_uniform = 17 + 3 * K
    sigma_of, normal = {}, {}

    def normal_row(row, s_flown, s_new, what):
        s_flown, s_new = float(s_flown), float(s_new)
        sigma_of[row] = s_flown
        if s_new == s_flown:
            return
        if s_flown == 0.0:
            raise ValueError(f"{what}: the flown sigma is 0 and the target is not - the run did not vary it, there is nothing to reweight")
        if not s_new > 0.0:
            raise ValueError(f"{what}: the target sigma is 0 - a point law has no density ratio to the flown one")
        normal[row] = [0.0, s_new / s_flown]

    for key, rows in _SIGMA_ROWS.items():
        for i, r in enumerate(rows):
            normal_row(r, base[key][i], new[key][i], f"{key}[{i}]")
    normal_row(12, base["mass_uncertainty"], new["mass_uncertainty"], "mass_uncertainty")
    for key in ("thrust_uncertainty", "atmospheric_density_uncertainty"):
        if new[key] != base[key]:
            raise ValueError(f"{key} of the uncertainty table has no primitive: its draw is dead (the motor's own thrust_uncertainty "
                             f"is the live one)")
    if motor is not None:
        tm = motor if target_motor is None else target_motor
        normal_row(14, motor.thrust_uncertainty, tm.thrust_uncertainty, "motor.thrust_uncertainty")
        if liquid:
            normal_row(15, motor.mass_flow_uncertainty, tm.mass_flow_uncertainty, "motor.mass_flow_uncertainty")
    elif target_motor is not None:
        raise ValueError("target_motor needs the flown `motor`")
    uniform = {}
    for key, row in (("wind_speed_range", first_uniform), ("wind_direction_range", first_uniform + 1)):
        lo, hi = (float(v) for v in base[key])
        lo2, hi2 = (float(v) for v in new[key])
        if (lo2, hi2) == (lo, hi):
            continue
        if not (lo <= lo2 < hi2 <= hi):
            raise ValueError(f"{key}: the target range [{lo2}, {hi2}] is not a range inside the flown [{lo}, {hi}] - weights cannot "
                             f"create samples where none were flown")
        uniform[row] = ((lo2 - lo) / (hi - lo), (hi2 - lo) / (hi - lo))
    names = scalar_primitives(K, liquid)
    dead = {13, 16} | (set() if liquid else {15})
    for name, mu in (shift or {}).items():
        row = names[name] if name in names else name
        if isinstance(row, str) or not 0 <= int(row) < first_uniform or int(row) in dead:
            raise ValueError(f"shift: {name!r} is neither a normal primitive of scalar_primitives nor the row of one")
        row = int(row)
        if sigma_of.get(row, 1.0) == 0.0:
            raise ValueError(f"shift: the flown sigma of {name!r} is 0 - the run did not vary it")
        normal.setdefault(row, [0.0, 1.0])[0] = float(mu)
    out = {}
    for row in sorted(set(normal) | set(uniform)):
        if planar and row in _PLANAR_ZEROED:
            continue
        if row in normal:
            if normal[row] != [0.0, 1.0]:
                out[row] = (_abi.DESIGN_NORMAL, normal[row][0], normal[row][1], 0.0, 1.0)
        else:
            out[row] = (_abi.DESIGN_UNIFORM, 0.0, 1.0) + uniform[row]
    if len(out) > _abi.RW_MAX_LAW:
        raise ValueError(f"{len(out)} primitive rows change, more than the {_abi.RW_MAX_LAW} erpl_mc_reweight takes: the effective sample "
                         f"size is a product over the rows and would be gone long before")
    return out


def check_groups(groups, n_rows):
    """`groups` as a list of (name, rows): at most 32, each non-empty, rows inside the primitive tensor, none shared."""
    items = [(str(name), [int(r) for r in rows]) for name, rows in dict(groups).items()]
    if not 1 <= len(items) <= _abi.SOBOL_MAX_FACTORS:
        raise ValueError(f"1 to {_abi.SOBOL_MAX_FACTORS} groups")
    seen = {}
    for name, rows in items:
        if not rows:
            raise ValueError(f"group {name!r} is empty")
        for r in rows:
            if not 0 <= r < n_rows:
                raise ValueError(f"group {name!r}: row {r} outside 0..{n_rows - 1}")
            if r in seen:
                raise ValueError(f"groups must be disjoint: row {r} is in {seen[r]!r} and in {name!r}")
            seen[r] = name
    return items


def pick_freeze_blocks(A, B, groups):
    """The k + 2 primitive tensors of the pick-freeze design of A and B ([rows, n] each), block by block: A, B, then for
    every group g of `groups` A with the rows of g taken from B.  A generator: one extra copy at a time."""
    if A.shape != B.shape:
        raise ValueError("A and B: the same shape")
    items = check_groups(groups, int(A.shape[0]))
    yield A
    yield B
    for _, rows in items:
        AB = A.clone()
        idx = torch.tensor(rows, dtype=torch.long, device=A.device)
        AB[idx] = B[idx]
        yield AB


def synthetic_dispersions(n, rocket, motor, wind_model, base_initial_conditions, device,
                          precision=_abi.PREC_F32, seed=1234, uncertainty=None,
                          base_altitude_profile=None, base_wind_profile=None, planar=False,
                          n_wind_knots=100, engine=None, draws=None):
    """n dispersed samples with the distributions of monte_carlo.py:156-179 / :225-288, drawn with
    torch's counter-based device generator straight into the SoA tensors the kernels read.

    The reference draws a sample's dispersions from `np.random.seed(i)`, its motor perturbation from a
    fresh `RandomState(i)` (monte_carlo.py:253, motor.py:95-125 / :171-186) and its wind turbulence
    from ANOTHER fresh `RandomState(i)` (monte_carlo.py:263, environment.py:161-198): three streams
    with the same seed, i.e. the same leading normals.  That joint law is kept here: one normal
    vector z per sample feeds all three consumers by position - z[0:14] the 14 dispersion normals
    (position, velocity, attitude, angular velocity, mass, thrust[dead]), z[0:2] (liquid) or z[0:3]
    (solid) the motor multipliers, z[3k + c] the turbulence innovation of knot k, component c.  The two
    uniforms (wind speed, direction) and the dead density draw are independent of it.

    Wind: with a base profile (CSV) -> baseline + AR(1) turbulence + uniform (speed, direction)
    offset (monte_carlo.py:268-280); otherwise the synthetic power-law profile on
    linspace(0, 25000, n_wind_knots) (monte_carlo.py:282-288).  The AR(1) recursion runs in fp64 in one
    HIP kernel (erpl_mc_synth_wind); the table is stored in the working precision.  `planar=True`
    zeroes every out-of-plane input (Set P).  Returns an engine.DeviceBatch resident on `device`.

    The draws are kept on the batch as `db.factors` (float64 [F, n] on the device) with `db.factor_names` (FACTOR_NAMES;
    no `motor_mass_flow_multiplier` row for a solid motor): position, velocity, attitude (Euler) and angular velocity
    as handed to the kernels, the mass multiplier, k_thrust, mdot / motor.mass_flow_rate, the two wind uniforms and
    the mean wind they give - the input of erpl_mc_correlation.  Mind the joint law above: with a non-zero
    `initial_position` sigma `position_x` is an exact affine image of `motor_thrust_multiplier` (both are z[0]) and
    `position_y` of the liquid mass-flow multiplier (z[1]) - the reference's behaviour, not a bug.  With the default
    sigma of 0 those columns are constant and the correlation drops them; otherwise its regression_ok = 0 says that
    the two effects cannot be told apart.

    draws: None (the joint law above, drawn here from `seed`), or a float64 [17 + 3 K + 2, n] device tensor of primitives
    (`primitive_draws`) for an INDEPENDENT law: rows 0..13 the dispersion normals (row 13 the reference's dead thrust draw),
    rows 14..16 the motor normals, rows 17..17 + 3 K - 1 the turbulence normals (knot k, component c at 17 + 3 k + c), the
    last two rows the uniforms in [0, 1) of wind speed and direction; `seed` is not used.  This is a deliberate deviation
    from the reference, for the variance-based sensitivity analysis alone (MonteCarloAnalyzer.sobol_indices): a
    pick-freeze design needs factors that can be frozen one at a time, and under the joint law z[0] is the thrust
    multiplier, `position_x` and the first turbulence innovation at once."""
    import ctypes as C

    import numpy as np
    reject_overrides(wind_model, "wind_model")
    u = dict(DEFAULT_UNCERTAINTY)
    if uncertainty:
        u.update(uncertainty)
    device = torch.device(device)
    f64 = torch.float64
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    if engine is None:
        from .simulator import shared_engine
        engine = shared_engine(device)

    def col(v):
        return torch.tensor(v, dtype=f64, device=device).view(3, 1)

    use_base = base_wind_profile is not None and base_altitude_profile is not None
    alt_np = (np.asarray(base_altitude_profile, dtype=np.float64) if use_base
              else np.linspace(0, 25000, n_wind_knots))
    K = len(alt_np)
    if K > _abi.MAX_WIND_KNOTS:
        raise _abi.ErplError(f"{K} wind knots exceed the ABI limit {_abi.MAX_WIND_KNOTS}")
    if draws is None:
        rows = max(3 * K, 14)
        z = torch.randn((rows, n), generator=gen, dtype=f64, device=device)   # the shared normal stream
        uni = torch.rand((2, n), generator=gen, dtype=f64, device=device)
        z_motor, z_wind = z, z
    else:
        if not (torch.is_tensor(draws) and draws.device == device and draws.dtype == f64
                and tuple(draws.shape) == (primitive_rows(K), n)):
            raise ValueError(f"draws must be a float64 [{primitive_rows(K)}, {n}] tensor on {device}: 17 + 3 K + 2 rows")
        z, z_motor, z_wind, uni = draws[0:14], draws[14:17], draws[17:17 + 3 * K], draws[17 + 3 * K:]

    ic0 = base_initial_conditions
    pos = col(ic0.get("position", [0.0] * 3)) + col(u["initial_position"]) * z[0:3]
    vel = col(ic0.get("velocity", [0.0] * 3)) + col(u["initial_velocity"]) * z[3:6]
    att = col(ic0.get("attitude", [0.0] * 3)) + col(u["initial_attitude"]) * z[6:9]
    omg = col(ic0.get("angular_velocity", [0.0] * 3)) + col(u["initial_angular_velocity"]) * z[9:12]
    mass_mult = 1.0 + u["mass_uncertainty"] * z[12]
    lo, hi = u["wind_speed_range"]
    wind_speed = lo + (hi - lo) * uni[0]
    lo, hi = u["wind_direction_range"]
    wind_dir = lo + (hi - lo) * uni[1]
    if planar:
        keep_v = col([1.0, 0.0, 1.0])
        keep_a = col([0.0, 1.0, 0.0])
        vel = col(ic0.get("velocity", [0.0] * 3)) * (1 - keep_v) + vel * keep_v
        att = col(ic0.get("attitude", [0.0] * 3)) * (1 - keep_a) + att * keep_a
        omg = omg * keep_a
    ic = torch.cat([pos, vel, _euler_to_quaternion(att[0], att[1], att[2]), omg]).contiguous()

    dry = rocket.dry_mass * mass_mult
    prop = rocket.propellant_mass * mass_mult
    rk = torch.stack([dry, prop]).contiguous()

    # motor perturbation (motor.py:95-125 / :171-186) + re-sync of burn time (monte_carlo.py:258-260)
    k_thrust = 1.0 + motor.thrust_uncertainty * z_motor[0]
    if motor_kind(motor) == _abi.MOTOR_SOLID:   # z[1], z[2]: burn-time and impulse multipliers, drawn then overwritten / unused
        mdot = 4.26 * k_thrust
        row0 = k_thrust
        ae = motor.nozzle_exit_area * k_thrust
    else:
        mdot = motor.mass_flow_rate * (1.0 + motor.mass_flow_uncertainty * z_motor[1])
        row0 = motor.thrust_vacuum * k_thrust
        ae = (motor.thrust_vacuum * k_thrust - motor.thrust_sea_level * k_thrust) / 101325.0
    burn = prop / mdot
    mt = torch.stack([row0, ae, mdot, burn]).contiguous()

    # wind: per-knot constants on the host exactly as the bit-exact generator computes them, AR(1) on the device
    sigma, rho, innov = knot_constants(wind_model, alt_np)
    dev64 = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=f64, device=device)
    sigma_d, rho_d, innov_d = dev64(sigma), dev64([0.0] + list(rho[1:])), dev64([0.0] + list(innov[1:]))
    if use_base:
        base_np = np.array(base_wind_profile, dtype=np.float64)
        if planar:
            base_np[:, 1] = 0.0
        base_d = dev64(base_np).contiguous()
        scale_d = torch.ones((K,), dtype=f64, device=device)
    else:
        base_d = None
        scale_d = dev64([(np.float64(a) / 10.0) ** wind_model.power_law_exponent for a in alt_np])  # environment.py:118-123
    mean_u = (wind_speed * torch.cos(wind_dir)).contiguous()
    mean_v = (torch.zeros_like(wind_speed) if planar else wind_speed * torch.sin(wind_dir)).contiguous()
    g = z_wind[: 3 * K].contiguous()
    if planar:
        g = g.clone()
        g.view(K, 3, n)[:, 1, :] = 0.0      # no cross-wind turbulence either
    wdt = torch.float32 if precision == _abi.PREC_F32 else f64
    wind = torch.empty((K, 3, n), dtype=wdt, device=device)
    st = torch.cuda.current_stream(device)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = engine.lib.erpl_mc_synth_wind(engine._ctx, n, K, ptr(g), ptr(sigma_d), ptr(rho_d), ptr(innov_d), ptr(base_d),
                                       ptr(scale_d), ptr(mean_u), ptr(mean_v), ptr(wind), int(precision),
                                       C.c_void_p(st.cuda_stream))
    _abi.check(engine.lib, rc, "erpl_mc_synth_wind")
    _check_ranges(ic, rk, mt, mean_u, mean_v)
    db = DeviceBatch(ic, rk, mt, dev64(alt_np).contiguous(), wind, precision)
    liquid = motor_kind(motor) != _abi.MOTOR_SOLID
    rows = [pos, vel, att, omg, mass_mult.view(1, n), k_thrust.view(1, n)]
    if liquid:
        rows.append((mdot / motor.mass_flow_rate).view(1, n))
    rows += [wind_speed.view(1, n), wind_dir.view(1, n), mean_u.view(1, n), mean_v.view(1, n)]
    db.factors = torch.cat([r.expand(r.shape[0], n) for r in rows]).contiguous()
    db.factor_names = [k for k in FACTOR_NAMES if liquid or k != "motor_mass_flow_multiplier"]
    return db
