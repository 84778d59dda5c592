// erpl_k_rail.h — kernel 1: the launch rail of every sample, and the fresh record of the resume queue it leaves.
namespace {

// ------------------------------------------------------------------------------------ kernel 1
// Launch rail, simulator.py:42-125: 1-D explicit Euler along body-x at dt_initial.
__global__ __launch_bounds__(256) void ERPL_CAT(erpl_rail_, ERPL_SUFFIX)(const ErplKArgs a, const ErplScalars<real> S) {
  __shared__ LdsTables L;
  __shared__ real alt_s[ERPL_MAX_WIND_KNOTS];
  stage_tables(L, alt_s, a.tables, a.alt_grid, a.k_wind);
  if (blockIdx.x == 0) {
    // this batch's queue cursors and counters start from zero (qcnt and qhead are one allocation); the flight
    // launches that use them come after this kernel on the stream - two fill dispatches per batch less
    for (int k = threadIdx.x; k < 2 * (ERPL_MAX_PHASES + 2) + 2 * ERPL_EXT_Q; k += blockDim.x) a.qcnt[k] = 0ull;   // (+ the hand-over queue's)
    if (threadIdx.x < 16) a.counters[threadIdx.x] = 0ull;
  }
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int64_t n = a.n;
  a.status[i] = ERPL_ST_INCOMPLETE;   // replaced when the trajectory ends (lane_finish)
  Shared C;
  C.S = &S;
  C.L = &L; C.alt = alt_s; C.has_wind = a.k_wind > 0; C.motor_kind = a.motor_kind;
  LaneParams p;
  p.dry = (real)a.rocket[0 * n + i]; p.prop = (real)a.rocket[1 * n + i];
  p.thrust = (real)a.motor[0 * n + i]; p.Ae = (real)a.motor[1 * n + i];
  p.mdot = (real)a.motor[2 * n + i]; p.burn = a.motor[3 * n + i];
  lane_params_finish(S, p);
  real pos[3], vel[3], q[4], om[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { pos[c] = (real)a.ic[c * n + i]; vel[c] = (real)a.ic[(3 + c) * n + i]; om[c] = (real)a.ic[(10 + c) * n + i]; }
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] = (real)a.ic[(6 + c) * n + i];
  // direction = R(q)[:, 0] with q normalised (utils.py:100-111)
  real w = q[0], x = q[1], yy = q[2], z = q[3];
  {
    const real nrm = m_sqrt(((w * w + x * x) + yy * yy) + z * z);
    if (nrm > (real)1e-12) { w = w / nrm; x = x / nrm; yy = yy / nrm; z = z / nrm; }
    else { w = 1; x = 0; yy = 0; z = 0; }
  }
  const real R00 = 1 - 2 * (yy * yy + z * z), R01 = 2 * (x * yy - w * z), R02 = 2 * (x * z + w * yy);
  const real R10 = 2 * (x * yy + w * z), R11 = 1 - 2 * (x * x + z * z), R12 = 2 * (yy * z - w * x);
  const real R20 = 2 * (x * z - w * yy), R21 = 2 * (yy * z + w * x), R22 = 1 - 2 * (x * x + yy * yy);
  const real d0 = R00, d1 = R10, d2 = R20;
  WindCache wc;
  wc.lo = 1; wc.hi = 0; wc.x0 = 0;  // empty interval -> first lookup loads
#pragma unroll
  for (int c = 0; c < 3; ++c) { wc.y0[c] = 0; wc.s[c] = 0; }
  MachCache mc;
  mach_cache_clear(mc);
  real distance = 0, pf = 1;
  double t = 0.0;
  const double dt = a.dt_rail;
  int nrail = 0;
  // (the iteration cap only guards against a non-finite burn time, which the reference would
  //  spin on forever; the host layer rejects such inputs before they get here)
  while (distance < S.rail_length && t < p.burn && nrail < (1 << 22)) {
    real mass, cg, Ixx, Iyy;
    mass_props(S, p, pf, mass, cg, Ixx, Iyy);
    real Tm, P;
    atmosphere(S, pos[2], Tm, P);
    const real rho = m_div(P, S.Rg * Tm);
    real wv[3];
    wind_at(C, i, pos[2], wc, wv);
    real speed = (vel[0] * d0 + vel[1] * d1) + vel[2] * d2;
    const real rv0 = d0 * speed - wv[0], rv1 = d1 * speed - wv[1], rv2 = d2 * speed - wv[2];
    const real rel_speed = (rv0 * d0 + rv1 * d1) + rv2 * d2;
    const real mach = m_div(m_sqrt((rv0 * rv0 + rv1 * rv1) + rv2 * rv2), m_sqrt((real)(1.4 * 287.053) * Tm));
    mach_lookup(C, mach, mc);
    const real* rec = mach_rec_of(C, mc);
    const real mq = (mach > kBig) ? kBig : mach;
    const real cd = (rec[2] * (mq - rec[0]) + rec[1]) + (rec[4] * (mq - rec[0]) + rec[3]) * (real)0;
    const real drag = ((((real)0.5 * rho) * (rel_speed * rel_speed)) * cd) * S.ref_area;
    real thrust = 0;  // motor.get_thrust(t, P): zero outside [0, burn_time]
    if (!(t < 0.0 || t > p.burn)) {
      if (C.motor_kind == ERPL_MOTOR_SOLID) thrust = solid_curve(C, (real)t, p.thrust) + p.Ae * ((real)101325.0 - P);
      else thrust = p.thrust - p.Ae * P;
    }
    const real g = gravity_at(S, pos[2]);
    const real accel = m_div((thrust - mass * g) - drag, mass);
    speed += accel * S.dt_rail;
    pos[0] += (d0 * speed) * S.dt_rail; pos[1] += (d1 * speed) * S.dt_rail; pos[2] += (d2 * speed) * S.dt_rail;
    distance += speed * S.dt_rail;
    vel[0] = d0 * speed; vel[1] = d1 * speed; vel[2] = d2 * speed;
    t += dt;
    ++nrail;
    // motor.get_propellant_remaining (motor.py:86-93 / :163-169)
    if (t <= 0.0) pf = 1;
    else if (t >= p.burn) pf = 0;
    else { const real r = (real)(1.0 - t / p.burn); pf = (r > 0) ? r : (real)0; }
  }
  // rail-exit diagnostics (:103-123)
  real wv[3];
  wind_at(C, i, pos[2], wc, wv);
  const real vr0 = vel[0] - wv[0], vr1 = vel[1] - wv[1], vr2 = vel[2] - wv[2];
  const real vb0 = (R00 * vr0 + R10 * vr1) + R20 * vr2;
  const real vb1 = (R01 * vr0 + R11 * vr1) + R21 * vr2;
  const real vb2 = (R02 * vr0 + R12 * vr1) + R22 * vr2;
  const bool a_dead = (m_abs(vb0) < (real)1e-6) && (m_abs(vb2) < (real)1e-6);
  const real vxz = m_sqrt(vb0 * vb0 + vb2 * vb2);
  const real aoa = a_dead ? (real)0 : m_atan2(vb2, vb0);
  const real ssl = (vxz < (real)1e-6) ? (real)0 : m_atan2(vb1, vxz);
  a.summary[ERPL_SUM_RAIL_EXIT_TIME * n + i] = t;
  a.summary[ERPL_SUM_RAIL_EXIT_SPEED * n + i] = (double)m_sqrt((vel[0] * vel[0] + vel[1] * vel[1]) + vel[2] * vel[2]);
  a.summary[ERPL_SUM_RAIL_EXIT_AOA * n + i] = (double)aoa;
  a.summary[ERPL_SUM_RAIL_EXIT_SIDESLIP * n + i] = (double)ssl;
  // park the rail-exit state as a fresh record of the resume queue (phase 0 pops records 0..n-1)
  {
    real* rr = (real*)a.res_r[0];
    double* rd = a.res_d[0];
    int32_t* ri = a.res_i[0];
    const int64_t cap = a.res_cap;
#pragma unroll
    for (int c = 0; c < 3; ++c) { rr[c * cap + i] = pos[c]; rr[(3 + c) * cap + i] = vel[c]; rr[(10 + c) * cap + i] = om[c]; }
#pragma unroll
    for (int c = 0; c < 4; ++c) rr[(6 + c) * cap + i] = q[c];
    rr[13 * cap + i] = pf;
    const real sp2 = (vel[0] * vel[0] + vel[1] * vel[1]) + vel[2] * vel[2];
    rr[14 * cap + i] = pos[2];                      // apogee so far: altitudes[0] (simulator.py:212-213)
    rr[15 * cap + i] = pos[2];
    rr[16 * cap + i] = (sp2 != sp2) ? (real)0 : sp2;
    rr[17 * cap + i] = 0; rr[18 * cap + i] = 0; rr[19 * cap + i] = 0;
    rd[0 * cap + i] = t; rd[1 * cap + i] = t; rd[2 * cap + i] = t; rd[3 * cap + i] = t; rd[4 * cap + i] = 0.0;
    ri[0 * cap + i] = (int32_t)i; ri[1 * cap + i] = 0; ri[2 * cap + i] = nrail;
    ri[3 * cap + i] = (kPhysics << 8) | kRecFresh | ((pos[2] != pos[2]) ? kRecNanSeen : 0);
    ri[4 * cap + i] = 0;
    ri[5 * cap + i] = 0; a.res_i[1][5 * cap + i] = 0;   // nothing published yet in either queue buffer
  }
}

}  // namespace
