// erpl_k_rhs_fast.h — the RHS of the two throughput builds: the same equations in the short formulation.
namespace {

// environment.py:26-103 through the lane's layer record (erpl_tables.h): temperature, its reciprocal
// and pressure.
__device__ __forceinline__ void fast_atmosphere(const Shared& C, const AtmCache& ac, real h, real& T, real& rT, real& P) {
#if ERPL_FAST_F64
  real r[10];
  {
    const RealPair* q = lds_record(C.L->atm, ac.ro);
#pragma unroll
    for (int k = 0; k < 5; ++k) { const RealPair v = q[k]; r[2 * k] = v.x; r[2 * k + 1] = v.y; }
  }
#else
  (void)C;
  const real* r = ac.r;
#endif
  const real aT = r[0], bT = r[1], Tlo = r[2], Thi = r[3];
  const real invTref = r[4], eL = r[5], href = r[6], eH = r[7], eM = r[8], pbase = r[9];
  T = m_clamp(bT + aT * h, Tlo, Thi);
  rT = m_rcp(T);
  P = pbase * m_exp2(eL * m_log2(T * invTref, h) + (h - href) * (eH + eM * rT), h);
}

// Rocket.get_aerodynamic_coefficients + get_dynamic_cp (rocket.py:138-218, :105-108) of the fast path:
// cd, cl, cy and cma = -cl_alpha * (cp - cg), so that cm = cma * alpha, cyaw = cma * beta.
__device__ __forceinline__ void fast_aero(const ErplScalars<real>& S, const real* rec, real mach, real mach2,
                                          real alpha, real beta, real pf, real cg, real& cd, real& cl, real& cy,
                                          real& cma) {
  const real mq = m_clamp(mach, (real)0, kBig);  // mach is finite or +inf here (q_dynamic > 0)
  const real dm = mq - rec[0];
  const real cd0 = rec[2] * dm + rec[1];
  const real cda = rec[4] * dm + rec[3];
  const real cps = rec[7] * (mq - rec[5]) + rec[6];
  cd = cd0 + cda * (alpha * alpha);
  cd = (pf > 0) ? cd : cd * S.power_off;
  const real abs_alpha = m_abs(alpha);
  // rocket.py:179-181: (AR beta / cos)^2 with beta = sqrt|1 - M^2| needs no square root
  const real cl_alpha = S.two_pi_AR_cos * m_rcp((real)2 + m_sqrt_pos((real)4 + S.AR_over_cos2 * m_abs((real)1 - mach2)));
  cy = cl_alpha * beta;
  {  // stall model (rocket.py:183-187, :203-205) as pure min/max arithmetic (no selects):
     // below the stall angle over = 0 -> sf = 1, cd factor = 1, cl = cl_alpha * alpha exactly
    const real over = m_max(abs_alpha - S.stall_angle, (real)0);
    const real sf = m_max((real)1 - over * S.inv_stall_span, (real)0);
    cd *= (real)1 + ((real)0.5 * over) * S.inv_stall_span;
    cy *= sf;
#if ERPL_FAST_F64
    cl = cl_alpha * m_copysign(m_clamp_abs_uniform(alpha, S.stall_angle) * sf, alpha);    // min(|alpha|, stall)
#else
    cl = cl_alpha * m_copysign(m_clamp(abs_alpha, (real)-1, S.stall_angle) * sf, alpha);  // min(|alpha|, stall)
#endif
  }
  const real sm = (S.cp_location + cps) - cg;
  cma = -cl_alpha * sm;
}

// Fast RHS: the same equations as the faithful rocket_dynamics() (simulator.py:295-460) with
// algebraically identical shortcuts (one reciprocal per denominator, rsq for 1/sqrt, cos/sin(atan2)
// as ratios, croll == 0 and Izz == Iyy used explicitly, the atmosphere layers as one exp2/log2 formula
// over a per-layer coefficient record).  The vector-ALU issue port is the resource this kernel runs
// out of, so the code is written for a short instruction stream: the
// altitude-keyed records sit in registers behind one range test, small conditionals are min / max /
// med3 / copysign arithmetic rather than compare+select pairs, and only blocks that are rare for the
// whole wave (parachute, table reloads) are branches.  NaN/inf propagation follows the reference's
// comparisons.
// The time of the evaluation enters in two places only: the burn gate `t <= burn_time` (:359) and the thrust
// curve's abscissa.  GATED = the caller has evaluated both for the stage (the flight kernel does it for the
// three stage times of a step at once, in fp64, so that no double is live across the stages).
template <bool GATED>
__device__ __forceinline__ void rocket_dynamics_at(const Shared& C, LaneParams& p, int64_t id,
                                                   WindCache& wc, MachCache& mc, AtmCache& ac, bool& chute, double t,
                                                   bool gate_le_burn, real gate_t,
                                                   const real (&y)[14], real (&dy)[14], StampSums& ss,
                                                   const LaneRec lr) {
  const ErplScalars<real>& S = *C.S;
  const real h = y[2];
  if (!(h >= ac.lo && h < ac.hi)) {  // rare
    ERPL_RARE_BLOCK();
    lr.wind_bounds(wc);   // the reload keeps the wind interval when only the atmosphere layer changed:
    lr.wind(wc);          // the whole record must be in hand before it is written back
    altitude_tables_reload(C, id, h, wc, ac);
    lr.put_wind(wc);
  }
  lr.fence();
  lr.wind(wc);
  real wv[3] = {0, 0, 0};
  if (C.has_wind) {  // wave-uniform
    const real d = m_clamp(h, -kBig, kBig) - wc.x0;  // NaN altitude: finite winds here, but rho (and so every use of them) is NaN
    wv[0] = wc.s[0] * d + wc.y0[0]; wv[1] = wc.s[1] * d + wc.y0[1]; wv[2] = wc.s[2] * d + wc.y0[2];
  }
  ERPL_STAMP(ss.seg[1], ss.last);
  // ---- attitude ----
  // Select diet (v_cmp / v_cndmask cost ~4.1 cycles each on the saturated vector port): where a
  // NaN can only occur in a state that is already non-finite - and therefore leaves the physics loop
  // through the NaN paths below - v_max / v_min / copysign forms replace compare+select pairs, and
  // guards that cannot trigger for the finite positive masses / inertias the host validates are
  // dropped: the identity-quaternion reset (utils.py:79-82), mass < dry_mass (:315-318), `if I > 0`
  // (:431-436).  The fp64 gate kernel keeps every one of them.
  const real pf = m_max(y[13], (real)0);  // max(0.0, pf): NaN -> 0, like Python's max (:305)
  // attitude: s = sqrt(2) q/|q|, so that every product s_i s_j is the 2 q_i q_j of utils.py:100-111
  real q0, q1, q2, q3;
  {
    const real r = m_rsq((((y[6] * y[6] + y[7] * y[7]) + y[8] * y[8]) + y[9] * y[9]) * (real)0.5);
    q0 = y[6] * r; q1 = y[7] * r; q2 = y[8] * r; q3 = y[9] * r;
  }
  const real q11 = q1 * q1, q22 = q2 * q2, q33 = q3 * q3;
  const real R00 = ((real)1 - q22) - q33, R01 = q1 * q2 - q0 * q3, R02 = q1 * q3 + q0 * q2;
  const real R10 = q1 * q2 + q0 * q3, R11 = ((real)1 - q11) - q33, R12 = q2 * q3 - q0 * q1;
  const real R20 = q1 * q3 - q0 * q2, R21 = q2 * q3 + q0 * q1, R22 = ((real)1 - q11) - q22;
  // ---- mass properties (rocket.py:110-136) ----
  const real mp = p.prop * pf;
  const real mass = p.dry + mp;
  const real rm = m_rcp(mass);
  const real cg = (p.dry_cg + mp * S.prop_cg) * rm;
  const real Ixx = S.Ixx_dry + mp * S.dq2;
  const real dcg = S.prop_cg - cg;
  const real Iyy = S.Iyy_dry + mp * (S.third + dcg * dcg);
  const real ri = m_rcp(Iyy);
  // ---- atmosphere, continued ----
  // the clamp drops a NaN temperature, but a NaN altitude still reaches P through (h - href), and
  // every consumer of T alone sits behind q_dynamic > 0
  real T, rT, P;
  fast_atmosphere(C, ac, h, T, rT, P);
  // ---- relative wind in body axes (:341-352) ----
  const real vr0 = y[3] - wv[0], vr1 = y[4] - wv[1], vr2 = y[5] - wv[2];
  const real vb0 = (R00 * vr0 + R10 * vr1) + R20 * vr2;
  const real vb1 = (R01 * vr0 + R11 * vr1) + R21 * vr2;
  const real vb2 = (R02 * vr0 + R12 * vr1) + R22 * vr2;
  const real vn2 = (vr0 * vr0 + vr1 * vr1) + vr2 * vr2;
  // Mach^2 = |v|^2 / (gamma R T) (utils.py:152-157); q = rho |v|^2 / 2 with rho = P / (R T) (:352,
  // environment.py:96) is the same product as (gamma/2) P Mach^2 - no density on the hot path
  const real mach2 = (vn2 * rT) * (real)(1.0 / (1.4 * 287.053));
  const real qdyn = (S.q_of_PM2 * P) * mach2;
  // ---- thrust (:359-363) ----
  // (the motor models give no thrust and no mass flow at t < 0 either: motor.py:54-57 / :152-153)
  const bool burning = (pf > 0) && (GATED ? gate_le_burn : (t >= 0.0 && t <= p.burn));
  real thrust;
  if (C.motor_kind == ERPL_MOTOR_SOLID) {  // wave-uniform
    thrust = burning ? solid_curve(C, GATED ? gate_t : (real)t, p.thrust) + p.Ae * ((real)101325.0 - P) : (real)0;
  } else {
    thrust = burning ? p.thrust - p.Ae * P : (real)0;
  }
#if ERPL_FAST_F64
  // The sums of the lateral forces and of the moments start from zero - but as initialisers ahead of the two branches the
  // zeros cost four 64-bit moves in every evaluation, for the lanes that skip the aerodynamic block: in flight next to none.
  // Here every path sets them: the aerodynamic block adds to a CONSTANT zero (m_add_zero: the same addition, x + 0 is not x
  // for x = -0), and the lanes it is not for - parachute out, or nothing to push against - write their zeros in a block of
  // their own, which the wave skips when it has no such lane and which holds the parachute drag.
  real fb0 = thrust, fb1, fb2, mb1, mb2;
#define ERPL_SUM_FROM_ZERO(v_, x_) v_ = m_add_zero(x_)
#else
  real fb0 = thrust, fb1 = 0, fb2 = 0, mb1 = 0, mb2 = 0;
#define ERPL_SUM_FROM_ZERO(v_, x_) v_ += x_
#endif
  ERPL_STAMP(ss.seg[2], ss.last);
  // ---- parachute latch (:366-369) and drag (:372-377) ----
  // A wave-skipped branch, not selects: the parachute is out in <1 % of all evaluations, and on this
  // kernel the vector-ALU port is the saturated resource (tools/ubench/valu_issue.hip: v_cmp and
  // v_cndmask cost ~4.1 cycles each per SIMD vs ~2.7 for an FMA) - measured -5 % time.  The other
  // small conditionals stay predicated: as branches they cost more (phi copies, exec bookkeeping).
  if (h <= S.chute_alt) { if (!chute && y[5] < 0) chute = true; }  // below 500 m only
#if ERPL_FAST_F64
  const bool aero = !chute && qdyn > 0;
  if (!aero) {
    ERPL_RARE_BLOCK();
    fb1 = 0; fb2 = 0;
    mb1 = m_zero_here(); mb2 = m_zero_here();   // (as plain constants the compiler hoists these two back ahead of the branch)
#endif
  if (chute) {
    const real rs2 = (vb0 * vb0 + vb1 * vb1) + vb2 * vb2;
    const real rs = m_sqrt(rs2);
    if (rs > 0) {
      const real rho = (P * S.inv_Rg) * rT;
      const real kc = -(rho * rs2) * S.chute_k * m_rcp(rs);
      fb0 += kc * vb0; fb1 += kc * vb1; fb2 += kc * vb2;
    }
  }
#if ERPL_FAST_F64
  }
  if (aero) {  // aerodynamics (:378-411, rocket.py:138-218)
#else
  if (!chute && qdyn > 0) {  // aerodynamics (:378-411, rocket.py:138-218)
#endif
    const real vxz2 = m_max(vb0 * vb0 + vb2 * vb2, (real)1e-30);
    const real rxz = m_rsq(vxz2);
    // The |v_body| < 1e-6 m/s dead zones of utils.py:160-172 force alpha/beta to 0 there; here the
    // denominators are floored instead (atan2(0,0) = 0, no NaN): for speeds below 1e-6 m/s the
    // aerodynamic force is < 1e-12 N either way, 15 orders below thrust and weight.
    const real vxz = vxz2 * rxz;  // rxz uses the floored vxz2 below
    const real v2f = m_max(vxz2 + vb1 * vb1, (real)1e-30);
    const real rv = m_rsq(v2f);
    real alpha, beta;
    m_aero_angles(vb2, vb0, vxz, vb1, vxz, v2f * rv, h, alpha, beta);
    const real ca = vb0 * rxz;
    const real sa = vb2 * rxz;
    const real cb = vxz * rv;
    const real sb = vb1 * rv;
    const real mach = m_sqrt_pos(mach2);   // q_dynamic > 0: mach2 > 0
    if (!mach_inside(C, mc, mach)) { ERPL_RARE_BLOCK(); mach_reload(C, mach, mc); }  // rare, divergent
    real cd, cl, cy, cma;
#if ERPL_FAST_F64
    real mrec[ERPL_MACH_REC];
    mach_rec_load(C, mc, mrec);
#else
    const real* mrec = mach_rec_of(C, mc);
#endif
    fast_aero(S, mrec, mach, mach2, alpha, beta, pf, cg, cd, cl, cy, cma);
    const real qs = qdyn * S.ref_area;
    const real drag = qs * cd, lift = qs * cl, side = qs * cy;
    fb0 += (sb * side - (ca * cb) * drag) - (sa * cb) * lift;
    ERPL_SUM_FROM_ZERO(fb1, (-(ca * sb) * drag - cb * side) - (sa * sb) * lift);
    ERPL_SUM_FROM_ZERO(fb2, sa * drag - ca * lift);
    const real qsd = qdyn * S.area_diam;
    mb1 = qsd * (cma * alpha);
    mb2 = qsd * (cma * beta);
  }
#undef ERPL_SUM_FROM_ZERO
  ERPL_STAMP(ss.seg[3], ss.last);
  const real wx = y[10], wy = y[11], wz = y[12];
  mb1 -= S.pitch_damping * wy;  // :414-415
  mb2 -= S.yaw_damping * wz;
  const real fi0 = (R00 * fb0 + R01 * fb1) + R02 * fb2;  // :418
  const real fi1 = (R10 * fb0 + R11 * fb1) + R12 * fb2;
  real fi2 = (R20 * fb0 + R21 * fb1) + R22 * fb2;
  {
    const real re = (real)6.371e6;
    const real r = re * m_rcp(re + h);
    fi2 -= mass * (S.g0 * (r * r));  // :421-422, environment.py:105-108
  }
  dy[0] = y[3]; dy[1] = y[4]; dy[2] = y[5];
  dy[3] = fi0 * rm; dy[4] = fi1 * rm; dy[5] = fi2 * rm;
  const real dI = Ixx - Iyy;  // Izz == Iyy (rocket.py:128); croll == 0 -> roll acceleration is 0
  dy[10] = 0;
  dy[11] = (mb1 - (dI * wz) * wx) * ri;  // :431-436
  dy[12] = (mb2 + (dI * wx) * wy) * ri;
  {  // quaternion kinematics (utils.py:114-121) on s = sqrt(2) q/|q|: 0.5 Omega(w) q = (0.5/sqrt 2) Omega(w) s.
     // The drift term -0.5 (|q|^2 - 1) q of :119-121 is evaluated on the normalised quaternion by the
     // reference, i.e. it is exactly 0 in exact arithmetic: dropped here (the fp64 kernel keeps it).
    const real c = (real)0.35355339059327376220;
    dy[6] = c * ((-(q1 * wx) - q2 * wy) - q3 * wz);
    dy[7] = c * ((q0 * wx + q2 * wz) - q3 * wy);
    dy[8] = c * ((q0 * wy - q1 * wz) + q3 * wx);
    dy[9] = c * ((q0 * wz + q1 * wy) - q2 * wx);
  }
  // propellant consumption with the burn-out clamp (:442-450)
  const real pfr = (pf * p.inv_abs_pfr < (real)0.01) ? pf * (real)-100.0 : p.pfr0;
  dy[13] = burning ? pfr : (real)0;
  ERPL_STAMP(ss.seg[4], ss.last);
}
__device__ __forceinline__ void rocket_dynamics(const Shared& C, LaneParams& p, int64_t id,
                                                WindCache& wc, MachCache& mc, AtmCache& ac, bool& chute, double t,
                                                const real (&y)[14], real (&dy)[14], StampSums& ss,
                                                const LaneRec lr) {
  rocket_dynamics_at<false>(C, p, id, wc, mc, ac, chute, t, false, (real)0, y, dy, ss, lr);
}

}  // namespace
