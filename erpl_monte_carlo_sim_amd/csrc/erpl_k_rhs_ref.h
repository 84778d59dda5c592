// erpl_k_rhs_ref.h — the RHS of the gate build (ERPL_FAITHFUL): simulator.py:295-460 in the reference's operation order.
namespace {

// Rocket.get_aerodynamic_coefficients + get_dynamic_cp (rocket.py:138-218, :105-108) in the
// reference's operation order; rec = np.interp records of the lane's Mach interval.
__device__ __forceinline__ void aero_coefficients(const ErplScalars<real>& S, const real* rec, real mach,
                                                  real alpha, real beta, real cg, bool power_on, real& cd,
                                                  real& cl, real& cy, real& cm, real& cyaw, real& cp_dyn) {
  const real mq = (mach > kBig) ? kBig : mach;
  const real cd0 = rec[2] * (mq - rec[0]) + rec[1];
  const real cda = rec[4] * (mq - rec[0]) + rec[3];
  const real cps = rec[7] * (mq - rec[5]) + rec[6];
  cd = cd0 + cda * (alpha * alpha);
  if (!power_on) cd *= S.power_off;
  const real abs_alpha = m_abs(alpha);
  const real beta_m = m_sqrt(m_abs((real)1 - mach * mach));
  const real arb = (S.AR * beta_m) / S.cos_sweep_c;
  const real denom = (real)2 + m_sqrt((real)4 + arb * arb);
  const real cl_alpha = m_div(S.two_pi_AR, denom) * S.cos_sweep;
  cl = cl_alpha * alpha;
  cy = cl_alpha * beta;
  if (abs_alpha > S.stall_angle) {
    const real over = abs_alpha - S.stall_angle;
    real sf = (real)1 - over / (S.max_angle - S.stall_angle);
    const real cdk = (real)1 + ((real)0.5 * over) / (S.max_angle - S.stall_angle);
    sf = (sf > 0) ? sf : (real)0;
    const real sgn = (alpha > 0) ? (real)1 : ((alpha < 0) ? (real)-1 : alpha);
    cl = ((cl_alpha * S.stall_angle) * sf) * sgn;
    cd *= cdk;
    cy *= sf;
  }
  cp_dyn = S.cp_location + cps;
  const real sm = cp_dyn - cg;
  cm = ((-cl_alpha) * sm) * alpha;
  cyaw = ((-cl_alpha) * sm) * beta;
}


// simulator.py:295-460.  `chute` is FlightSimulator.parachute_deployed, latched in here (so it
// can trip at an RK trial state).
__device__ __forceinline__ void rocket_dynamics(const Shared& C, const LaneParams& p, int64_t id,
                                                WindCache& wc, MachCache& mc, AtmCache& ac, bool& chute, double t,
                                                const real (&y)[14], real (&dy)[14], StampSums& ss) {
  (void)ss; (void)ac;
  const ErplScalars<real>& S = *C.S;
  const real pf = (y[13] > 0) ? y[13] : (real)0;  // max(0.0, pf), NaN -> 0   (:305)
  // normalize_quaternion (utils.py:76-82)
  real q0 = y[6], q1 = y[7], q2 = y[8], q3 = y[9];
  {
    const real nrm = m_sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    if (nrm > (real)1e-12) {
      if (kFaithful) { q0 = q0 / nrm; q1 = q1 / nrm; q2 = q2 / nrm; q3 = q3 / nrm; }
      else { const real r = m_rcp(nrm); q0 *= r; q1 *= r; q2 *= r; q3 *= r; }
    } else { q0 = 1; q1 = 0; q2 = 0; q3 = 0; }
  }
  real mass, cg, Ixx, Iyy;
  mass_props(S, p, pf, mass, cg, Ixx, Iyy);
  if (mass < p.dry) {  // :315-318 (unreachable for finite inputs; kept for NaN/negative masses)
    LaneParams p0 = p;
    mass_props(S, p0, (real)0, mass, cg, Ixx, Iyy);
    mass = p.dry;
  }
  const real Izz = Iyy;  // rocket.py:128
  // quaternion_to_rotation_matrix (utils.py:100-111) normalises once more
  real w = q0, x = q1, yy = q2, z = q3;
  if (kFaithful) {
    const real nrm = m_sqrt(((w * w + x * x) + yy * yy) + z * z);
    if (nrm > (real)1e-12) { w = w / nrm; x = x / nrm; yy = yy / nrm; z = z / nrm; }
    else { w = 1; x = 0; yy = 0; z = 0; }
  }
  const real R00 = 1 - 2 * (yy * yy + z * z), R01 = 2 * (x * yy - w * z), R02 = 2 * (x * z + w * yy);
  const real R10 = 2 * (x * yy + w * z), R11 = 1 - 2 * (x * x + z * z), R12 = 2 * (yy * z - w * x);
  const real R20 = 2 * (x * z - w * yy), R21 = 2 * (yy * z + w * x), R22 = 1 - 2 * (x * x + yy * yy);
  const real h = y[2];
  real T, P;
  atmosphere(S, h, T, P);
  const real rho = m_div(P, S.Rg * T);
  real wv[3];
  wind_at(C, id, h, wc, wv);
  const real vr0 = y[3] - wv[0], vr1 = y[4] - wv[1], vr2 = y[5] - wv[2];
  const real vb0 = (R00 * vr0 + R10 * vr1) + R20 * vr2;  // R^T v_rel   (:344)
  const real vb1 = (R01 * vr0 + R11 * vr1) + R21 * vr2;
  const real vb2 = (R02 * vr0 + R12 * vr1) + R22 * vr2;
  const real vn2 = (vr0 * vr0 + vr1 * vr1) + vr2 * vr2;
  const real vn = m_sqrt(vn2);
  const real mach = m_div(vn, m_sqrt((real)(1.4 * 287.053) * T));  // utils.py:152-157
  const real qdyn = kFaithful ? ((real)0.5 * rho) * (vn * vn) : ((real)0.5 * rho) * vn2;  // :352
  // thrust (:359-363, motor.py:54-76 / :152-156)
  // (motor.py:54-57 / :152-153 gate thrust and mass flow with `time < 0 or time > burn_time`: t <= burn_time is :359, t >= 0 theirs)
  const bool burning = (pf > 0) && (t >= 0.0) && (t <= p.burn);
  real thrust = 0;
  if (burning) {
    if (C.motor_kind == ERPL_MOTOR_SOLID) thrust = solid_curve(C, (real)t, p.thrust) + p.Ae * ((real)101325.0 - P);
    else thrust = p.thrust - p.Ae * P;
  }
  real fb0 = thrust, fb1 = 0, fb2 = 0, mb0 = 0, mb1 = 0, mb2 = 0;
  // parachute latch (:366-369)
  if (h <= S.chute_alt) { if (!chute && y[5] < 0) chute = true; }  // below 500 m only
  if (chute) {  // :372-377
    const real rs = m_sqrt((vb0 * vb0 + vb1 * vb1) + vb2 * vb2);
    if (rs > 0) {
      real drag = (((real)0.5 * rho) * (rs * rs)) * S.chute_cd;
      drag *= S.chute_area;
      if (kFaithful) { fb0 += (-drag * vb0) / rs; fb1 += (-drag * vb1) / rs; fb2 += (-drag * vb2) / rs; }
      else { const real k = -drag * m_rcp(rs); fb0 += k * vb0; fb1 += k * vb1; fb2 += k * vb2; }
    }
  } else if (qdyn > 0) {  // :378-411, rocket.py:138-218
    // aerodynamic angles (utils.py:160-172) and the wind->body rotation (utils.py:175-205)
    real alpha, beta, ca, sa, cb, sb;
    const real vxz2 = vb0 * vb0 + vb2 * vb2;
    const real vxz = m_sqrt(vxz2);
    const bool a_dead = (m_abs(vb0) < (real)1e-6) && (m_abs(vb2) < (real)1e-6);
    const bool b_dead = vxz < (real)1e-6;
    alpha = a_dead ? (real)0 : m_atan2(vb2, vb0);
    beta = b_dead ? (real)0 : m_atan2(vb1, vxz);
    if (kFaithful) {
      sincos(alpha, &sa, &ca); sincos(beta, &sb, &cb);   // one argument reduction for both (same values as sin / cos)
    } else {  // cos/sin(atan2(b, a)) = a/r, b/r
      const real rxz = m_rcp(vxz);
      ca = a_dead ? (real)1 : vb0 * rxz;
      sa = a_dead ? (real)0 : vb2 * rxz;
      const real rv = m_rcp(m_sqrt(vxz2 + vb1 * vb1));
      cb = b_dead ? (real)1 : vxz * rv;
      sb = b_dead ? (real)0 : vb1 * rv;
    }
    mach_lookup(C, mach, mc);
    real cd, cl, cy, cm, cyaw, cp_dyn;
    aero_coefficients(S, mach_rec_of(C, mc), mach, alpha, beta, cg, pf > 0, cd, cl, cy, cm, cyaw, cp_dyn);
    const real drag = (qdyn * cd) * S.ref_area;
    const real lift = (qdyn * cl) * S.ref_area;
    const real side = (qdyn * cy) * S.ref_area;
    if (kFaithful) {
      fb0 += (((ca * cb) * (-drag)) + ((-sb) * (-side))) + ((sa * cb) * (-lift));
      fb1 += (((ca * sb) * (-drag)) + (cb * (-side))) + ((sa * sb) * (-lift));
      fb2 += (((-sa) * (-drag)) + ((real)0 * (-side))) + (ca * (-lift));
      mb0 += ((qdyn * (real)0) * S.ref_area) * S.ref_diam;
    } else {
      fb0 += (sb * side - (ca * cb) * drag) - (sa * cb) * lift;
      fb1 += (-(ca * sb) * drag - cb * side) - (sa * sb) * lift;
      fb2 += sa * drag - ca * lift;
    }
    mb1 += ((qdyn * cm) * S.ref_area) * S.ref_diam;
    mb2 += ((qdyn * cyaw) * S.ref_area) * S.ref_diam;
  }
  mb1 += -S.pitch_damping * y[11];  // :414-415
  mb2 += -S.yaw_damping * y[12];
  real fi0 = (R00 * fb0 + R01 * fb1) + R02 * fb2;  // :418
  real fi1 = (R10 * fb0 + R11 * fb1) + R12 * fb2;
  real fi2 = (R20 * fb0 + R21 * fb1) + R22 * fb2;
  fi2 -= mass * gravity_at(S, h);  // :421-422
  const real wx = y[10], wy = y[11], wz = y[12];
  dy[0] = y[3]; dy[1] = y[4]; dy[2] = y[5];
  if (kFaithful) {
    dy[3] = fi0 / mass; dy[4] = fi1 / mass; dy[5] = fi2 / mass;
    dy[10] = (Ixx > 0) ? (mb0 - ((Izz - Iyy) * wy) * wz) / Ixx : (real)0;  // :431-436
    dy[11] = (Iyy > 0) ? (mb1 - ((Ixx - Izz) * wz) * wx) / Iyy : (real)0;
    dy[12] = (Izz > 0) ? (mb2 - ((Iyy - Ixx) * wx) * wy) / Izz : (real)0;
  } else {
    const real rm = m_rcp(mass), ri = m_rcp(Iyy);
    dy[3] = fi0 * rm; dy[4] = fi1 * rm; dy[5] = fi2 * rm;
    dy[10] = (Ixx > 0) ? mb0 * m_rcp(Ixx) : (real)0;  // Izz == Iyy, croll == 0
    dy[11] = (Iyy > 0) ? (mb1 - ((Ixx - Izz) * wz) * wx) * ri : (real)0;
    dy[12] = (Izz > 0) ? (mb2 - ((Iyy - Ixx) * wx) * wy) * ri : (real)0;
  }
  // quaternion kinematics (utils.py:114-121) with the normalised q and omega_q = (0, w)
  {
    const real zero = 0;
    real m0, m1, m2, m3;
    if (kFaithful) {
      m0 = ((q0 * zero - q1 * wx) - q2 * wy) - q3 * wz;
      m1 = ((q0 * wx + q1 * zero) + q2 * wz) - q3 * wy;
      m2 = ((q0 * wy - q1 * wz) + q2 * zero) + q3 * wx;
      m3 = ((q0 * wz + q1 * wy) - q2 * wx) + q3 * zero;
    } else {
      m0 = (-(q1 * wx) - q2 * wy) - q3 * wz;
      m1 = (q0 * wx + q2 * wz) - q3 * wy;
      m2 = (q0 * wy - q1 * wz) + q3 * wx;
      m3 = (q0 * wz + q1 * wy) - q2 * wx;
    }
    const real ne = (((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3) - (real)1;
    const real k = (real)0.5 * ne;
    dy[6] = (real)0.5 * m0 - k * q0;
    dy[7] = (real)0.5 * m1 - k * q1;
    dy[8] = (real)0.5 * m2 - k * q2;
    dy[9] = (real)0.5 * m3 - k * q3;
  }
  // propellant consumption with the burn-out clamp (:442-450)
  real pfr = 0;
  if (burning) {
    pfr = m_div(-p.mdot, p.prop);
    const real remaining = (pfr != 0) ? m_div(pf, m_abs(pfr)) : (real)INFINITY;
    if (remaining < (real)0.01) pfr = m_div(-pf, (real)0.01);
  }
  dy[13] = pfr;
}

}  // namespace
