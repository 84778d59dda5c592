// erpl_k_debug.h — the evaluation of one stored record and kernel 3 on top of it (per-step diagnostic histories, gate build
// only), and the known-answer debug kernel.
namespace {

#if ERPL_FAITHFUL
// ------------------------------------------------------------------------------------ one stored record
// What FlightSimulator._extract_results evaluates for ONE stored state (simulator.py:511-552) besides the Euler angles,
// in the reference's operation order: mass properties, atmosphere, wind, relative velocity in the body frame, Mach,
// aerodynamic angles and coefficients, dynamic pressure, thrust at the rail-shifted time ts, drag and stability margin.
// Kernel 3 stores these per record; the envelope kernel (erpl_k_envelope.h) reduces them per trajectory.  The wind and
// Mach intervals are looked up afresh for every record: the values do not depend on what a thread evaluated before.
struct RecordEval {
  real mass, cg, Ixx, Iyy;
  real T, P, rho;
  real vb0, vb1, vb2, vn, mach;
  real alpha, beta;
  real cd, cl, cy, cm, cyaw, cp_dyn;
  real qdyn, thrust, drag, margin;
};
__device__ __forceinline__ void record_eval(const Shared& C, const LaneParams& p, int64_t id, double ts,
                                            const real (&y)[14], RecordEval& e) {
  const ErplScalars<real>& S = *C.S;
  mass_props(S, p, y[13], e.mass, e.cg, e.Ixx, e.Iyy);
  atmosphere(S, y[2], e.T, e.P);
  e.rho = e.P / (S.Rg * e.T);
  WindCache wc;
  wc.lo = 1; wc.hi = 0; wc.x0 = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) { wc.y0[c] = 0; wc.s[c] = 0; }
  real wv[3];
  wind_at(C, id, y[2], wc, wv);
  const real vr0 = y[3] - wv[0], vr1 = y[4] - wv[1], vr2 = y[5] - wv[2];
  real w = y[6], x = y[7], yy = y[8], z = y[9];
  {
    const real nrm = m_sqrt(((w * w + x * x) + yy * yy) + z * z);
    if (nrm > (real)1e-12) { w = w / nrm; x = x / nrm; yy = yy / nrm; z = z / nrm; }
    else { w = 1; x = 0; yy = 0; z = 0; }
  }
  const real R00 = 1 - 2 * (yy * yy + z * z), R01 = 2 * (x * yy - w * z), R02 = 2 * (x * z + w * yy);
  const real R10 = 2 * (x * yy + w * z), R11 = 1 - 2 * (x * x + z * z), R12 = 2 * (yy * z - w * x);
  const real R20 = 2 * (x * z - w * yy), R21 = 2 * (yy * z + w * x), R22 = 1 - 2 * (x * x + yy * yy);
  e.vb0 = (R00 * vr0 + R10 * vr1) + R20 * vr2;
  e.vb1 = (R01 * vr0 + R11 * vr1) + R21 * vr2;
  e.vb2 = (R02 * vr0 + R12 * vr1) + R22 * vr2;
  e.vn = m_sqrt((vr0 * vr0 + vr1 * vr1) + vr2 * vr2);
  e.mach = e.vn / m_sqrt((real)(1.4 * 287.053) * e.T);
  const bool a_dead = (m_abs(e.vb0) < (real)1e-6) && (m_abs(e.vb2) < (real)1e-6);
  const real vxz = m_sqrt(e.vb0 * e.vb0 + e.vb2 * e.vb2);
  e.alpha = a_dead ? (real)0 : m_atan2(e.vb2, e.vb0);
  e.beta = (vxz < (real)1e-6) ? (real)0 : m_atan2(e.vb1, vxz);
  MachCache mc;
  mach_cache_clear(mc);
  mach_lookup(C, e.mach, mc);
  aero_coefficients(S, mach_rec_of(C, mc), e.mach, e.alpha, e.beta, e.cg, y[13] > 0, e.cd, e.cl, e.cy, e.cm, e.cyaw, e.cp_dyn);
  e.qdyn = ((real)0.5 * e.rho) * (e.vn * e.vn);
  e.thrust = 0;  // motor.get_thrust(time[i], P) (motor.py:54-76 / :152-156)
  if (!(ts < 0.0 || ts > p.burn)) {
    if (C.motor_kind == ERPL_MOTOR_SOLID) e.thrust = solid_curve(C, (real)ts, p.thrust) + p.Ae * ((real)101325.0 - e.P);
    else e.thrust = p.thrust - p.Ae * e.P;
  }
  e.drag = (e.qdyn * e.cd) * S.ref_area;
  e.margin = (e.cp_dyn - e.cg) / S.ref_diam;
}

// The per-sample parameters of sample `id` of a batch of n, as the flight kernel's lanes load them.
__device__ __forceinline__ void lane_params_of(const ErplKArgs& a, const ErplScalars<real>& S, int64_t id, LaneParams& p) {
  const int64_t n = a.n;
  p.dry = (real)a.rocket[0 * n + id]; p.prop = (real)a.rocket[1 * n + id];
  p.thrust = (real)a.motor[0 * n + id]; p.Ae = (real)a.motor[1 * n + id];
  p.mdot = (real)a.motor[2 * n + id]; p.burn = a.motor[3 * n + id];
  lane_params_finish(S, p);
}

// ------------------------------------------------------------------------------------ kernel 3
// FlightSimulator._extract_results per-step loop (simulator.py:511-552): one thread per stored
// record of one trajectory.  a.traj = records [m][15], a.traj_cap = m, a.n_traj = sample index,
// a.summary = out [m][ERPL_DIAG_DIM].
__global__ __launch_bounds__(256) void erpl_extract_f64(const ErplKArgs a, const ErplScalars<real> S,
                                                        const double time_offset) {
  __shared__ LdsTables L;
  __shared__ real alt_s[ERPL_MAX_WIND_KNOTS];
  stage_tables(L, alt_s, a.tables, a.alt_grid, a.k_wind);
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.traj_cap) return;
  Shared C;
  C.S = &S; C.L = &L; C.alt = alt_s; C.has_wind = a.k_wind > 0; C.motor_kind = a.motor_kind;
  const int64_t id = a.n_traj;
  LaneParams p;
  lane_params_of(a, S, id, p);
  const double* rec = a.traj + r * ERPL_TRAJ_DIM;
  const double ts = rec[0] - time_offset;  // rail-shifted time (simulator.py:464, :543)
  real y[14];
#pragma unroll
  for (int c = 0; c < 14; ++c) y[c] = (real)rec[1 + c];
  double* o = a.summary + r * ERPL_DIAG_DIM;
  {  // quaternion_to_euler on the stored quaternion (utils.py:139-144 via :46-70)
    const real w = y[6], x = y[7], yy = y[8], z = y[9];
    o[0] = atan2(2 * (w * x + yy * z), 1 - 2 * (x * x + yy * yy));
    const real sinp = 2 * (w * yy - z * x);
    o[1] = (fabs(sinp) >= 1) ? copysign(1.57079632679489661923, sinp) : asin(sinp);
    o[2] = atan2(2 * (w * z + x * yy), 1 - 2 * (yy * yy + z * z));
  }
  RecordEval e;
  record_eval(C, p, id, ts, y, e);
  o[3] = e.cg; o[4] = e.mass; o[5] = e.Ixx; o[6] = e.Iyy; o[7] = e.Iyy;
  o[8] = e.thrust;
  o[9] = e.drag;
  o[10] = e.cd; o[11] = e.cl; o[12] = e.cm;
  o[13] = e.cp_dyn;
  o[14] = e.margin;
  o[15] = e.alpha; o[16] = e.beta;
}
#endif  // ERPL_FAITHFUL

// ------------------------------------------------------------------------------------ debug kernel
// Known-answer evaluation on the device (erpl_mc_debug_eval; tests only): ONE function of the hot path
// per lane, through the very device functions the flight kernel inlines.  Lane j takes the per-sample
// parameters and wind table of sample j % n; in / out are [rows][m] doubles.
//   ERPL_DBG_ATMOSPHERE  in: altitude                        out: T, P, rho, g
//   ERPL_DBG_AERO        in: mach, alpha, beta, pf, power_on out: cd, cl, cy, cm, cyaw
//   ERPL_DBG_RHS         in: t, y[14], chute                 out: dy[14], chute
//   ERPL_DBG_RHS_SEQ     as ERPL_DBG_RHS, but n lanes (one per sample): lane id evaluates the columns id, id + n,
//                        id + 2n, ... < m in that order through ONE set of wind / Mach / atmosphere caches (and LDS wind
//                        record) that is cleared before the first column only; the parachute latch comes from each
//                        column's input, so the expected values are those of ERPL_DBG_RHS
//   ERPL_DBG_MATH        in: x, y                            out: the ERPL_DBG_MATH_ROWS rows below, each through the
//                        m_* function of this build (erpl_k_math.h), NaN where the build has none:
//     0 m_rcp(x)            1 m_rsq(x)             2 m_sqrt_pos(x) (gate: m_sqrt)   3 m_exp2(x, x)
//     4 m_log2(x, x)        5 m_exp(x)             6 m_pow(x, y)                    7 m_div(x, y)
//     8 m_atan2(y, x)       9 m_clamp(x, -1, y)   10 alpha, 11 beta of m_aero_angles(y, x, r, y, |x|, r, x), r =
//    v2 m_rsq(v2), v2 = max(x^2 + y^2, 1e-30) as the fast RHS forms them     12, 13 alpha, beta once more through the single
//    m_atan2_half<false>(y, x, r, x), m_atan2_half<true>(y, |x|, r, x) (fp64 throughput build)
//    14 m_next_up(x)       15 m_sqrt(x)
//   ERPL_DBG_MINMAX      (fp64 throughput build only) in: x, y, z   out: the ERPL_DBG_MINMAX_ROWS rows below
//     0 m_max(x, y)         1 m_min(x, y)          2 m_clamp(x, y, z)               3 m_max(x, 0)
//     4 m_max(x, 1e-30)     5 m_clamp(x, -kBig, kBig)   6 m_clamp_abs_uniform(x, S.stall_angle)   7 m_add_zero(x)
__global__ __launch_bounds__(256) void ERPL_CAT(erpl_debug_, ERPL_SUFFIX)(const ErplKArgs a, const ErplScalars<real> S,
                                                                         const int what, const int64_t m,
                                                                         const double* __restrict__ in,
                                                                         double* __restrict__ out) {
  __shared__ LdsTables L;
  __shared__ real alt_s[ERPL_MAX_WIND_KNOTS];
  stage_tables(L, alt_s, a.tables, a.alt_grid, a.k_wind);
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = a.n;
  if (j >= ((what == ERPL_DBG_RHS_SEQ) ? n : m)) return;
  Shared C;
  C.S = &S; C.L = &L; C.alt = alt_s; C.has_wind = a.k_wind > 0; C.motor_kind = a.motor_kind;
  const int64_t id = j % n;   // (ERPL_DBG_RHS_SEQ: j < n, the lane's own sample)
  LaneParams p;
  p.dry = (real)a.rocket[0 * n + id]; p.prop = (real)a.rocket[1 * n + id];
  p.thrust = (real)a.motor[0 * n + id]; p.Ae = (real)a.motor[1 * n + id];
  p.mdot = (real)a.motor[2 * n + id]; p.burn = a.motor[3 * n + id];
  lane_params_finish(S, p);
  WindCache wc;
  wc.lo = 1; wc.hi = 0; wc.x0 = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) { wc.y0[c] = 0; wc.s[c] = 0; }
  MachCache mc;
  mach_cache_clear(mc);
  AtmCache ac;
  atm_cache_clear(ac);
#if !ERPL_FAITHFUL
  LaneRec lr;
#if ERPL_FAST_F64
  __shared__ real lane_wind[kLwSlots][kWave];   // launched with 64 threads per workgroup
  lr.lw = &lane_wind[0][threadIdx.x];
  lr.put_wind(wc);
#endif
#endif
  if (what == ERPL_DBG_ATMOSPHERE) {
    const real h = (real)in[j];
    real T, P, rho, g;
#if ERPL_FAITHFUL
    atmosphere(S, h, T, P);
    rho = m_div(P, S.Rg * T);
    g = gravity_at(S, h);
#else
    real rT;
    altitude_tables_reload(C, id, h, wc, ac);
    fast_atmosphere(C, ac, h, T, rT, P);
    rho = (P * S.inv_Rg) * rT;
    const real re = (real)6.371e6;
    const real r = re * m_rcp(re + h);
    g = S.g0 * (r * r);
#endif
    out[0 * m + j] = (double)T; out[1 * m + j] = (double)P; out[2 * m + j] = (double)rho; out[3 * m + j] = (double)g;
  } else if (what == ERPL_DBG_AERO) {
    const real mach = (real)in[0 * m + j], alpha = (real)in[1 * m + j], beta = (real)in[2 * m + j];
    const real pf = (real)in[3 * m + j];
    mach_lookup(C, mach, mc);
    real cd, cl, cy, cm, cyaw;
#if ERPL_FAITHFUL
    real mass, cg, Ixx, Iyy, cp_dyn;
    mass_props(S, p, pf, mass, cg, Ixx, Iyy);
    aero_coefficients(S, mach_rec_of(C, mc), mach, alpha, beta, cg, in[4 * m + j] > 0.0, cd, cl, cy, cm, cyaw, cp_dyn);
#else
    const real mp = p.prop * pf;
    const real cg = (p.dry_cg + mp * S.prop_cg) * m_rcp(p.dry + mp);
    real cma;
    fast_aero(S, mach_rec_of(C, mc), mach, mach * mach, alpha, beta, pf, cg, cd, cl, cy, cma);
    cm = cma * alpha; cyaw = cma * beta;
#endif
    out[0 * m + j] = (double)cd; out[1 * m + j] = (double)cl; out[2 * m + j] = (double)cy;
    out[3 * m + j] = (double)cm; out[4 * m + j] = (double)cyaw;
  } else if (what == ERPL_DBG_MATH) {
    const real x = (real)in[0 * m + j], y = (real)in[1 * m + j];
    real o[ERPL_DBG_MATH_ROWS];
#pragma unroll
    for (int k = 0; k < ERPL_DBG_MATH_ROWS; ++k) o[k] = (real)NAN;
    o[0] = m_rcp(x);
    o[5] = m_exp(x); o[6] = m_pow(x, y); o[7] = m_div(x, y); o[8] = m_atan2(y, x);
    o[14] = m_next_up(x); o[15] = m_sqrt(x);
#if ERPL_FAITHFUL
    o[2] = m_sqrt(x);
#else
    o[1] = m_rsq(x); o[2] = m_sqrt_pos(x);
    o[3] = m_exp2(x, x); o[4] = m_log2(x, x);
    o[9] = m_clamp(x, (real)-1, y);
    {  // the angles as rocket_dynamics_at calls them: the lengths are the floored sum of squares times its m_rsq
      const real v2 = m_max(x * x + y * y, (real)1e-30);
      const real r = v2 * m_rsq(v2);
      m_aero_angles(y, x, r, y, m_abs(x), r, x, o[10], o[11]);
#if ERPL_FAST_F64
      o[12] = m_atan2_half<false>(y, x, r, x);
      o[13] = m_atan2_half<true>(y, m_abs(x), r, x);
#endif
    }
#endif
#pragma unroll
    for (int k = 0; k < ERPL_DBG_MATH_ROWS; ++k) out[k * m + j] = (double)o[k];
#if ERPL_FAST_F64
  } else if (what == ERPL_DBG_MINMAX) {
    const real x = in[0 * m + j], y = in[1 * m + j], z = in[2 * m + j];
    out[0 * m + j] = m_max(x, y); out[1 * m + j] = m_min(x, y); out[2 * m + j] = m_clamp(x, y, z);
    out[3 * m + j] = m_max(x, (real)0); out[4 * m + j] = m_max(x, (real)1e-30); out[5 * m + j] = m_clamp(x, -kBig, kBig);
    out[6 * m + j] = m_clamp_abs_uniform(x, S.stall_angle); out[7 * m + j] = m_add_zero(x);
#endif
  } else {
    // ERPL_DBG_RHS: the one column j.  ERPL_DBG_RHS_SEQ: every n-th column from j on, the caches carried over.
    const int64_t stride = (what == ERPL_DBG_RHS_SEQ) ? n : m;
    for (int64_t col = j; col < m; col += stride) {
      const double t = in[0 * m + col];
      real y[14], dy[14];
#pragma unroll
      for (int c = 0; c < 14; ++c) y[c] = (real)in[(1 + c) * m + col];
      bool chute = in[15 * m + col] > 0.0;
      StampSums ss;
#if ERPL_FAITHFUL
      rocket_dynamics(C, p, id, wc, mc, ac, chute, t, y, dy, ss);
#else
      rocket_dynamics(C, p, id, wc, mc, ac, chute, t, y, dy, ss, lr);
#endif
#pragma unroll
      for (int c = 0; c < 14; ++c) out[c * m + col] = (double)dy[c];
      out[14 * m + col] = chute ? 1.0 : 0.0;
    }
  }
}

}  // namespace
