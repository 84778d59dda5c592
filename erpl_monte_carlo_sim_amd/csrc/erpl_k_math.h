// erpl_k_math.h — the m_* families: the working-precision wrappers every build uses, then the fast arithmetic of the
// fp64 throughput build (own exp2 / log2 / atan on coefficient tables) and of the fp32 build (hardware transcendentals).
namespace {

// ------------------------------------------------------------------------------------ math: every build
__device__ __forceinline__ double m_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ double m_exp(double x) { return exp(x); }
__device__ __forceinline__ double m_pow(double x, double y) { return pow(x, y); }
__device__ __forceinline__ double m_atan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ double m_abs(double x) { return fabs(x); }
__device__ __forceinline__ double m_div(double a, double b) { return a / b; }
#if !ERPL_FAST_F64
__device__ __forceinline__ double m_rcp(double a) { return 1.0 / a; }   // (the fp64 throughput build has its own below)
#endif
__device__ __forceinline__ float m_abs(float x) { return fabsf(x); }
// min / max / copysign in the working precision (NaN handling of fmin/fmax: the non-NaN operand)
__device__ __forceinline__ float m_max(float a, float b) { return fmaxf(a, b); }
#if !ERPL_FAST_F64
__device__ __forceinline__ double m_max(double a, double b) { return fmax(a, b); }   // (the fp64 throughput build has its own below)
#endif
__device__ __forceinline__ float m_copysign(float a, float b) { return copysignf(a, b); }
__device__ __forceinline__ double m_copysign(double a, double b) { return copysign(a, b); }
// smallest value above a positive finite x (half-open ranges over closed layer bounds)
__device__ __forceinline__ float m_next_up(float x) { return __int_as_float(__float_as_int(x) + 1); }
__device__ __forceinline__ double m_next_up(double x) { return __longlong_as_double(__double_as_longlong(x) + 1); }

template <typename T> __device__ __forceinline__ bool m_isnan(T x) { return x != x; }

constexpr real kBig = (real)1e30;  // clamp for table abscissae so that 0-slope * inf stays finite

#if ERPL_FAST_F64
// ------------------------------------------------------------------------------------ math: fp64 throughput build
// The polynomial coefficients of the fp64 throughput build's exp2 / log2 / atan.  Left to itself the compiler
// hoists every 64-bit coefficient out of the RK4 loop into VECTOR registers - ~50 doubles that it then spills to
// scratch and re-loads, or copies (v_mov_b64) before each accumulating v_fmac - the opposite of what a
// register-capped loop needs; materialised in scalar registers at their use (two s_mov each) they cost ~100
// scalar instructions per RHS evaluation, and with two waves per SIMD a wave still issues one instruction of ANY
// kind per slot (tools/ubench/f64_issue.hip).  So the coefficients sit in constant memory, one table per
// polynomial, and reach scalar registers by s_load_dwordx8 / x16 behind a laundered pointer (the loads cannot
// leave the loop); a Horner step is then one three-address v_fma_f64 with a scalar addend.
struct PolyTables {
  double exp2[16];   // 2^f, |f| <= 1/2: Taylor coefficients (ln 2)^k / k!, k = 13 .. 1
  double log2[16];   // (2/ln 2) / (2k+1), k = 11 .. 0
  double atan[16];   // fdlibm s_atan.c aT[10], aT[8] .. aT[0] (odd part), then aT[9], aT[7] .. aT[1]
};
__constant__ __attribute__((aligned(128))) PolyTables kPoly = {
  {1.3691488853904128e-12, 2.5678435993488206e-11, 4.4455382718708116e-10, 7.054911620801123e-09,
   1.01780860092397e-07, 1.321548679014431e-06, 1.5252733804059841e-05, 0.0001540353039338161,
   0.0013333558146428443, 0.009618129107628477, 0.05550410866482158, 0.24022650695910072,
   0.6931471805599453, 0, 0, 0},
  {0.12545174268599682, 0.1373995277037108, 0.15186263588304877, 0.16972882833987804, 0.19235933878519512,
   0.22195308321368667, 0.2623081892525388, 0.3205988979753252, 0.4121985831111324, 0.5770780163555853,
   0.9617966939259756, 2.8853900817779268, 0, 0, 0, 0},
  {1.62858201153657823623e-02, 4.97687799461593236017e-02, 6.66107313738753120669e-02, 9.09088713343650656196e-02,
   1.42857142725034663711e-01, 3.33333333333329318027e-01,
   -3.65315727442169155270e-02, -5.83357013379057348645e-02, -7.69187620504482999495e-02,
   -1.11111104054623557880e-01, -1.99999999998764832476e-01, 0, 0, 0, 0, 0}};
typedef const double __attribute__((address_space(4)))* PolyPtr;
__device__ __forceinline__ PolyPtr poly_table(const double* t, double arg) {
  PolyPtr q = (PolyPtr)t;
  asm("" : "+s"(q) : "v"(arg));
  return q;
}
// (each value passes through an empty asm with a scalar-register constraint: the operand folder does not fold a
// sub-register of the 16-dword load result into a VOP3 source by itself and would copy it to a vector register)
// `after`: the value the coefficient is about to be combined with - the (empty) asm then sits at the point of
// use and the wait for the load with it, behind the arithmetic that precedes it, not right behind the load.
// (not volatile: a pure function of a loop-variant value can be neither hoisted nor merged, and the scheduler
// stays free to interleave independent polynomials)
__device__ __forceinline__ double poly_coef(double c, double after) { asm("" : "+s"(c) : "v"(after)); return c; }
#define ERPL_POLY(name_, arg_) const PolyPtr pc = poly_table(kPoly.name_, arg_)
#define KS(i_, v_, after_) poly_coef(pc[i_], after_)   // v_: the value of kPoly.<name>[i_], written out for the reader
// v_rcp_f64 seed (measured on MI355X: 4.6e-8 relative, tools/ubench/f64_seed.hip) + ONE cubic round
// r (1 + e + e^2), e = 1 - a r: error e^3 ~ 1e-22, result within 1.0 ulp - the same as the two Newton rounds
// of round 2 at three FMAs instead of four.  No denormal / overflow scaling: fast-path operands are
// O(1e-6 .. 1e12); blow-ups go to inf/NaN as in the reference (0 and +-inf give NaN: e = 1 - 0 * inf).
// (The bounds of this file are asserted on the device against mpmath by tests/test_gpu_math.py; measured worst errors:
// DESIGN.md section 5.)
__device__ __forceinline__ double m_rcp(double a) {
  const double r = __builtin_amdgcn_rcp(a);
  const double e = __builtin_fma(-a, r, 1.0);
  return __builtin_fma(r, __builtin_fma(e, e, e), r);
}
// v_rsq_f64 seeds one cubic round like m_rcp above
__device__ __forceinline__ double m_rsq(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  // y <- y (1 + e/2 + 3 e^2/8), e = 1 - x y^2 : cubic convergence; the hardware seed is good to 5.2e-8, so ONE
  // round lands within 1.24 ulp - exactly where the second round of round 2 left it (tools/ubench/f64_seed.hip)
  const double e = __builtin_fma(-(x * y), y, 1.0);
  return __builtin_fma(y * e, __builtin_fma(0.375, e, 0.5), y);
}
// sqrt of a positive finite value as x rsq(x) (7 instructions; the library routine scales, fixes up and
// classifies: 17): within 2 * 1.24 + 0.5 = 2.98 ulp (the ulp of rsq(x) weighs up to two of the root's, and the product
// rounds once).  0 and +inf give NaN where sqrt gives 0 and +inf: both callers feed a state that is past saving.
__device__ __forceinline__ double m_sqrt_pos(double x) { return x * m_rsq(x); }
// max / min / clamp as ONE v_max_f64 / v_min_f64 each.  fmax / fmin first quiet every operand the compiler cannot prove free of
// signalling NaNs - a value read from LDS, a kernel argument, anything computed in another basic block - with a
// v_max_f64 x, x, x of its own (IEEE mode): 21 vector instructions per RK4 step.  The instruction itself already returns the
// other operand for a quiet NaN; the two forms differ for a SIGNALLING NaN alone (quieted here, dropped there), which no
// arithmetic instruction produces and the host refuses in the inputs.  Asserted bit for bit against numpy.fmax / fmin on the
// device by tests/test_gpu_step_diet_bits.py.  The second operand: a compile-time constant goes in as an inline constant
// (0, +-1) or through a scalar register pair, as the compiler folds it into fmax; anything else is a vector register.
// For a later caller: (1) the kernels run in IEEE mode (the default of a compute kernel; with it off the instruction passes a
// signalling NaN on unquieted); (2) put a constant SECOND - as the first operand it is copied into a vector pair; (3) whether
// b is a constant is decided after inlining (__builtin_constant_p on a parameter of a forced-inline function): at -O0 every
// call takes the vector form, which is right but moves constants through registers.
#define ERPL_MINMAX_F64(name_, op_)                                                                     \
  __device__ __forceinline__ double name_(double a, double b) {                                         \
    double r;                                                                                           \
    if (__builtin_constant_p(b)) {                                                                      \
      if (b == 0.0 && !__builtin_signbit(b)) asm(op_ " %0, %1, 0" : "=v"(r) : "v"(a));                  \
      else if (b == 1.0) asm(op_ " %0, %1, 1.0" : "=v"(r) : "v"(a));                                    \
      else if (b == -1.0) asm(op_ " %0, %1, -1.0" : "=v"(r) : "v"(a));                                  \
      else asm(op_ " %0, %1, %2" : "=v"(r) : "v"(a), "s"(b));                                           \
    } else {                                                                                            \
      asm(op_ " %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));                                                \
    }                                                                                                   \
    return r;                                                                                           \
  }
ERPL_MINMAX_F64(m_max, "v_max_f64")
ERPL_MINMAX_F64(m_min, "v_min_f64")
#undef ERPL_MINMAX_F64
__device__ __forceinline__ double m_clamp(double x, double lo, double hi) { return m_min(m_max(x, lo), hi); }
// m_clamp(|x|, -1, hi) with hi wave-uniform (a kernel argument): the source modifier and the scalar operand, which the
// compiler folds into fmax / fmin and cannot fold into an asm operand, written out.  UNIFORM ONLY: hi goes in through a
// scalar register, so of a lane-varying hi every lane would silently get the first active lane's - pass members of the
// by-value kernel arguments (S.*) or constants, nothing computed per lane.
__device__ __forceinline__ double m_clamp_abs_uniform(double x, double hi) {
  double r;
  asm("v_max_f64 %0, |%1|, -1.0\n\tv_min_f64 %0, %0, %2" : "=&v"(r) : "v"(x), "s"(hi));
  return r;
}
// 0 + x as the v_add_f64 it is when the zero is a register the compiler knows nothing about - written out, so that the
// contraction of x into FMAs is the one an unknown addend gets (a visible constant zero re-associates it)
__device__ __forceinline__ double m_add_zero(double x) {
  double r;
  asm("v_add_f64 %0, 0, %1" : "=v"(r) : "v"(x));
  return r;
}
// A zero written where the call stands: as a plain constant, the zero of a value that another path computes is moved ahead of
// the branch and paid for on every path
__device__ __forceinline__ double m_zero_here() {
  double r;
  asm volatile("v_mov_b64 %0, 0" : "=v"(r));
  return r;
}
// exp2 / log2 / atan for the operand ranges of this RHS, without the special-case ladders of a general
// libm (those cost ~40 % of its instructions, and with one wave per SIMD every instruction is 4 cycles);
// NaN in -> NaN out, results overflow / underflow to inf / 0 through v_ldexp_f64.  Errors: m_exp2 <= 2 ulp (denormal
// spacing below 2^-1022; integers exact); m_log2 and the angles are NOT within 2 ulp of the result - see each.
// 2^x: x = n + f, |f| <= 1/2, 2^f by the degree-13 Taylor polynomial of exp(f ln 2) (next term 4e-18).
__device__ __forceinline__ double m_exp2(double x, double early) {
  ERPL_POLY(exp2, early);
  x = (x < -1100.0) ? -1100.0 : x;   // -inf (pressure at an infinite altitude) -> 0, not inf - inf
  const double n = __builtin_rint(x);
  const double f = x - n;
  double p = KS(0, 1.3691488853904128e-12, f);
  p = __builtin_fma(p, f, KS(1, 2.5678435993488206e-11, f));   // (anchored on f: p is still a scalar here)
  p = __builtin_fma(p, f, KS(2, 4.4455382718708116e-10, p));
  p = __builtin_fma(p, f, KS(3, 7.054911620801123e-09, p));
  p = __builtin_fma(p, f, KS(4, 1.01780860092397e-07, p));
  p = __builtin_fma(p, f, KS(5, 1.321548679014431e-06, p));
  p = __builtin_fma(p, f, KS(6, 1.5252733804059841e-05, p));
  p = __builtin_fma(p, f, KS(7, 0.0001540353039338161, p));
  p = __builtin_fma(p, f, KS(8, 0.0013333558146428443, p));
  p = __builtin_fma(p, f, KS(9, 0.009618129107628477, p));
  p = __builtin_fma(p, f, KS(10, 0.05550410866482158, p));
  p = __builtin_fma(p, f, KS(11, 0.24022650695910072, p));
  p = __builtin_fma(p, f, KS(12, 0.6931471805599453, p));
  p = __builtin_fma(p, f, 1.0);
  return __builtin_amdgcn_ldexp(p, (int)n);
}
// log2 x, x > 0: x = 2^e m, m in [sqrt(1/2), sqrt 2), s = (m - 1)/(m + 1), |s| <= 0.1716,
// log2 m = (2/ln 2) s (1 + s^2/3 + s^4/5 + ... + s^22/23)   (next term 6e-19)
// Error: absolute, <= 1.5 ulp at max(|log2 x|, 1) (three roundings of O(ulp(1/2)) each in s q + e); in ulps of the
// result that is up to ~3 where |log2 x| is just below a power of two (3.04 measured just under sqrt 2), never above 4.
// Powers of two are exact (s == 0).
__device__ __forceinline__ double m_log2(double x, double early) {
  ERPL_POLY(log2, early);
  int e = __builtin_amdgcn_frexp_exp(x);
  double m = __builtin_amdgcn_frexp_mant(x);      // [1/2, 1)
  const bool small = m < 0.70710678118654752440;
  m = small ? m + m : m;
  e = small ? e - 1 : e;
  const double s = (m - 1.0) * m_rcp(m + 1.0);
  const double z = s * s;
  double q = KS(0, 0.12545174268599682, z);
  q = __builtin_fma(q, z, KS(1, 0.1373995277037108, z));   // (anchored on z: q is still a scalar here)
  q = __builtin_fma(q, z, KS(2, 0.15186263588304877, q));
  q = __builtin_fma(q, z, KS(3, 0.16972882833987804, q));
  q = __builtin_fma(q, z, KS(4, 0.19235933878519512, q));
  q = __builtin_fma(q, z, KS(5, 0.22195308321368667, q));
  q = __builtin_fma(q, z, KS(6, 0.2623081892525388, q));
  q = __builtin_fma(q, z, KS(7, 0.3205988979753252, q));
  q = __builtin_fma(q, z, KS(8, 0.4121985831111324, q));
  q = __builtin_fma(q, z, KS(9, 0.5770780163555853, q));
  q = __builtin_fma(q, z, KS(10, 0.9617966939259756, q));
  q = __builtin_fma(q, z, KS(11, 2.8853900817779268, q));
  return __builtin_fma(s, q, (double)e);
}
// The aerodynamic angles through the half angle, as m_atan2_half<float> above: atan2(y, |x|) =
// 2 atan(a), a = y / (r + |x|), |a| <= 1.  |a| > tan(pi/8) is folded once more with
// atan a = pi/4 + atan((a - 1)/(a + 1)) - written on numerator and denominator so that ONE reciprocal
// serves both cases - and the remaining |t| <= 0.4142 takes the 11-term minimax polynomial of fdlibm's
// s_atan.c (valid to 7/16, < 1 ulp).  The angle as a whole - reciprocal, fold, pi/4 and the doubling on top of the
// polynomial, and the rounding of the length r the caller supplies - is within 4 ulp of the result (3.0 measured, on the
// fold), not 2: about 5e-16 rad.
template <bool XPOS>
__device__ __forceinline__ double m_atan2_half(double y, double x, double r, double early) {
  ERPL_POLY(atan, early);
  const double ay = fabs(y), den = r + fabs(x);
  const bool big = ay > 0.41421356237309503 * den;
  const double num = big ? ay - den : ay;
  const double dn = big ? ay + den : den;
  const double t = num * m_rcp(dn);
  const double z = t * t, w = z * z;
  double s1 = KS(0, 1.62858201153657823623e-02, w);
  double s2 = KS(6, -3.65315727442169155270e-02, w);
  s1 = __builtin_fma(s1, w, KS(1, 4.97687799461593236017e-02, w));   // (anchored on w: s1, s2 are still scalars here)
  s2 = __builtin_fma(s2, w, KS(7, -5.83357013379057348645e-02, w));
  s1 = __builtin_fma(s1, w, KS(2, 6.66107313738753120669e-02, s1));
  s2 = __builtin_fma(s2, w, KS(8, -7.69187620504482999495e-02, s2));
  s1 = __builtin_fma(s1, w, KS(3, 9.09088713343650656196e-02, s1));
  s2 = __builtin_fma(s2, w, KS(9, -1.11111104054623557880e-01, s2));
  s1 = __builtin_fma(s1, w, KS(4, 1.42857142725034663711e-01, s1));
  s2 = __builtin_fma(s2, w, KS(10, -1.99999999998764832476e-01, s2));
  s1 = __builtin_fma(s1, w, KS(5, 3.33333333333329318027e-01, s1));
  const double corr = t * __builtin_fma(s1, z, s2 * w);      // t (z s1 + w s2)
  double a = (big ? 0.78539816339744830962 : 0.0) + (t - corr);
  a = a + a;                                                    // |atan2(y, |x|)|
  if (!XPOS) a = (x < 0.0) ? 3.14159265358979323846 - a : a;
  return copysign(a, y);
}
// Both aerodynamic angles at once: alpha = atan2(ya, xa) (any xa), beta = atan2(yb, xb) (xb >= 0) with ra, rb the
// lengths supplied by the caller.  Same arithmetic as two m_atan2_half calls; the coefficients are fetched once
// and the four Horner chains are written interleaved (fp64 FMAs have a dependent-issue latency of two issue slots).
__device__ __forceinline__ void m_atan2_half_pair(double ya, double xa, double ra, double yb, double xb, double rb,
                                                  double early, double& alpha, double& beta) {
  ERPL_POLY(atan, early);
  const double aya = fabs(ya), dena = ra + fabs(xa);
  const double ayb = fabs(yb), denb = rb + fabs(xb);
  const bool biga = aya > 0.41421356237309503 * dena;
  const bool bigb = ayb > 0.41421356237309503 * denb;
  const double numa = biga ? aya - dena : aya, dna = biga ? aya + dena : dena;
  const double numb = bigb ? ayb - denb : ayb, dnb = bigb ? ayb + denb : denb;
  const double ta = numa * m_rcp(dna), tb = numb * m_rcp(dnb);
  const double za = ta * ta, zb = tb * tb, wa = za * za, wb = zb * zb;
  const double c0 = KS(0, 1.62858201153657823623e-02, wa), c6 = KS(6, -3.65315727442169155270e-02, wa);
  double s1a = c0, s2a = c6, s1b = c0, s2b = c6;
  // (a1_, a2_: what the coefficients are anchored on - the chain values, except in the first step, where s1a and s2a
  // are still the scalars c0 and c6 and an anchor on them would be a dead copy into vector registers)
#define ERPL_ATAN_STEP(i1_, v1_, i2_, v2_, a1_, a2_)                          \
  {                                                                           \
    const double k1 = KS(i1_, v1_, a1_), k2 = KS(i2_, v2_, a2_);              \
    s1a = __builtin_fma(s1a, wa, k1); s2a = __builtin_fma(s2a, wa, k2);       \
    s1b = __builtin_fma(s1b, wb, k1); s2b = __builtin_fma(s2b, wb, k2);       \
  }
  ERPL_ATAN_STEP(1, 4.97687799461593236017e-02, 7, -5.83357013379057348645e-02, wa, wa)
  ERPL_ATAN_STEP(2, 6.66107313738753120669e-02, 8, -7.69187620504482999495e-02, s1a, s2a)
  ERPL_ATAN_STEP(3, 9.09088713343650656196e-02, 9, -1.11111104054623557880e-01, s1a, s2a)
  ERPL_ATAN_STEP(4, 1.42857142725034663711e-01, 10, -1.99999999998764832476e-01, s1a, s2a)
#undef ERPL_ATAN_STEP
  {
    const double k1 = KS(5, 3.33333333333329318027e-01, s1a);
    s1a = __builtin_fma(s1a, wa, k1);
    s1b = __builtin_fma(s1b, wb, k1);
  }
  const double corra = ta * __builtin_fma(s1a, za, s2a * wa), corrb = tb * __builtin_fma(s1b, zb, s2b * wb);
  double a = (biga ? 0.78539816339744830962 : 0.0) + (ta - corra);
  double b = (bigb ? 0.78539816339744830962 : 0.0) + (tb - corrb);
  a = a + a; b = b + b;
  a = (xa < 0.0) ? 3.14159265358979323846 - a : a;
  alpha = copysign(a, ya);
  beta = copysign(b, yb);
}
__device__ __forceinline__ void m_aero_angles(double ya, double xa, double ra, double yb, double xb, double rb, double early,
                                              double& alpha, double& beta) {
  m_atan2_half_pair(ya, xa, ra, yb, xb, rb, early, alpha, beta);
}
#endif  // ERPL_FAST_F64

#if ERPL_FAST_F32
// ------------------------------------------------------------------------------------ math: fp32 throughput build
// Hardware transcendental instructions (1 ulp v_rcp/v_sqrt/v_rsq/v_exp/v_log), no denormal or
// range fix-up code.  Inputs on this path are O(1e-6 .. 1e8); blow-ups go to inf/NaN as in fp64.
__device__ __forceinline__ float m_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float m_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float m_pow(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }
__device__ __forceinline__ float m_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float m_rcp(float a) { return __builtin_amdgcn_rcpf(a); }
// atan2 for finite, not-both-zero arguments: octant reduction + odd minimax polynomial on [0,1], NaN-propagating.
// |error| <= 4.5e-8 rad (the polynomial's own 4.44e-8) + 2.8 ulp of the result (reciprocal, quotient and the
// pi/2 / pi reflections): fp32 angles past 2 rad are 2.4e-7 rad apart, the worst measured is 2.9e-7 rad at 2.57 rad.
__device__ __forceinline__ float m_atan2(float y, float x) {
  float ax = fabsf(x), ay = fabsf(y);
  float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  float a = mn * __builtin_amdgcn_rcpf(mx);
  float s = a * a;
  // odd minimax polynomial a + a*s*(c0 + c1 s + ... + c7 s^7), Estrin scheme: depth 4 instead of 8
  const float s2 = s * s, s4 = s2 * s2;
  const float p01 = fmaf(0.199926957488059997558594f, s, -0.333331018686294555664062f);
  const float p23 = fmaf(0.106347933411598205566406f, s, -0.142027363181114196777344f);
  const float p45 = fmaf(0.0425049886107444763183594f, s, -0.0748900920152664184570312f);
  const float p67 = fmaf(0.00282363896258175373077393f, s, -0.0159569028764963150024414f);
  const float p03 = fmaf(p23, s2, p01);
  const float p47 = fmaf(p67, s2, p45);
  float r = fmaf(p47, s4, p03);
  r = fmaf(r * s, a, a);
  r = (ay > ax) ? 1.57079632679489661923f - r : r;
  r = (x < 0.0f) ? 3.14159265358979323846f - r : r;
  r = (x != x || y != y) ? (x + y) : r;  // NaN in -> NaN out (fmax/fmin drop a NaN beside a number: mx, mn cannot tell)
  return copysignf(r, y);
}
// Aerodynamic angles of the fast RHS through the half angle: with r = sqrt(x^2 + y^2) supplied by the
// caller (floored > 0, so atan2(0, 0) = 0: the dead zone of utils.py:160-172),
//   atan2(y, |x|) = 2 atan(y / (r + |x|)),  |y / (r + |x|)| <= 1,
// so the [0,1] polynomial applies without octant reduction (no min/max, no pi/2 fix-up) and the sign
// of y comes with the quotient.  Arguments are finite (q_dynamic > 0 has been tested).  XPOS: x >= 0.
// Coefficients are twice those of m_atan2: |error| <= 9e-8 rad (twice the polynomial's) + 3.5 ulp of the result
// (3.7e-7 rad measured at 1.59 rad, where an fp32 ulp is 1.2e-7 rad).
template <bool XPOS>
__device__ __forceinline__ float m_atan2_half(float y, float x, float r, float /*early*/) {
  const float a = y * __builtin_amdgcn_rcpf(r + fabsf(x));
  const float s = a * a;
  const float s2 = s * s, s4 = s2 * s2;
  const float p01 = fmaf(2.0f * 0.199926957488059997558594f, s, 2.0f * -0.333331018686294555664062f);
  const float p23 = fmaf(2.0f * 0.106347933411598205566406f, s, 2.0f * -0.142027363181114196777344f);
  const float p45 = fmaf(2.0f * 0.0425049886107444763183594f, s, 2.0f * -0.0748900920152664184570312f);
  const float p67 = fmaf(2.0f * 0.00282363896258175373077393f, s, 2.0f * -0.0159569028764963150024414f);
  float t = a * fmaf(fmaf(fmaf(p67, s2, p45), s4, fmaf(p23, s2, p01)), s, 2.0f);
  if (!XPOS) t = (x < 0.0f) ? copysignf(3.14159265358979323846f, y) - t : t;
  return t;
}
// clamp / min of loaded values as ONE v_med3_f32: fminf/fmaxf first quiet their operands (v_max x, x)
// in IEEE mode when the compiler cannot prove them free of signalling NaNs.  A NaN x gives lo.
__device__ __forceinline__ float m_clamp(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }
__device__ __forceinline__ float m_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float m_sqrt_pos(float x) { return m_sqrt(x); }
__device__ __forceinline__ float m_exp2(float x, float /*early*/) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float m_log2(float x, float /*early*/) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ void m_aero_angles(float ya, float xa, float ra, float yb, float xb, float rb, float early,
                                              float& alpha, float& beta) {
  alpha = m_atan2_half<false>(ya, xa, ra, early);
  beta = m_atan2_half<true>(yb, xb, rb, early);
}
#endif  // ERPL_FAST_F32

}  // namespace
