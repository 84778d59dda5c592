// erpl_kernels.inc — the trajectory kernels, written once and compiled three times:
//   erpl_k64.hip  : real = double, ERPL_FAITHFUL = 1, -ffp-contract=off  (correctness gate, cfg 2; one wave per SIMD; the
//                   same instantiation finishes the blow-ups the fp64 throughput build hands over: ERPL_SWEEP_MINW)
//   erpl_k64f.hip : real = double, ERPL_FAITHFUL = 0, ERPL_TWO_WAVE = 1   (fp64 throughput: the headline build)
//   erpl_k32.hip  : real = float,  ERPL_FAITHFUL = 0                      (fp32 throughput: healthy flights / first apogee)
//
// One trajectory per lane (wave64).  Kernel 1 integrates the launch rail (simulator.py:42-125)
// for every sample and parks the rail-exit state as a record of the resume queue.  Kernel 2 is the
// flight integrator (simulator.py:208-264 over _rocket_dynamics :295-460): every wave pops lane
// records from a device-wide atomic queue, keeps the 14-state, the per-sample parameters and the
// current wind / Mach-table / atmosphere intervals in registers (the two-wave fp64 build: the state and the
// wind interval in per-lane LDS, the table records by index in the workgroup's LDS tables), reads the shared
// interval tables only when a lane leaves its interval, and uses wave ballots to refill finished lanes from
// the queue, to hand the last lanes of a thinning wave to fuller waves (lane adoption) and (with step-chunked
// launches) to park still-flying lanes densely for the next launch.  Kernel 3 (fp64 only) evaluates the
// per-step diagnostic histories of _extract_results (:496-552).
//
// ERPL_FAITHFUL = 1 keeps the reference's operation order (double normalisation, trig of
// atan2, IEEE divisions); = 0 allows algebraically identical shortcuts (no trig, reciprocal
// multiplies, hardware transcendental instructions).  Reference citations are on each block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "erpl_tables.h"

#ifndef ERPL_REAL
#error "define ERPL_REAL, ERPL_FAITHFUL and ERPL_LAUNCH_NAME before including"
#endif

#ifndef ERPL_FAST_F64
#define ERPL_FAST_F64 0
#endif
#ifndef ERPL_FAST_F32
#define ERPL_FAST_F32 0
#endif
#ifndef ERPL_TWO_WAVE
#define ERPL_TWO_WAVE 0   // fp64 throughput build: two waves per SIMD (described below)
#endif
#ifndef ERPL_OCML_TRANSCENDENTALS
#define ERPL_OCML_TRANSCENDENTALS 0   // 1: the fp64 fast path calls the device library's exp2 / log2 / atan2 (A/B only)
#endif

typedef ERPL_REAL real;
// Precision of the integrated STATE (and of the altitude trackers derived from it).  The shipped
// builds integrate in the working precision; -DERPL_STATE_F64=1 on the fp32 unit is the
// "mixed" experiment of DESIGN.md section 5 (fp32 RHS, fp64 state and RK4 combination).
#ifndef ERPL_STATE_F64
#define ERPL_STATE_F64 0
#endif
#if ERPL_STATE_F64
typedef double state_t;
#else
typedef ERPL_REAL state_t;
#endif
// trajectories that can no longer change anything but x, y, t advance step by step (exact reference
// rounding) when the state is fp64, in closed form when it is fp32
#define ERPL_STEP_COAST (ERPL_FAITHFUL || ERPL_FAST_F64)
// Where the uniform constants of the RK4 loop live.  fp32: scalar registers straight from the kernel
// arguments.  fp64 constants take two SGPRs each and the 57 of them do not fit next to everything else:
// the compiler evicts and RE-LOADS them inside the loop (scalar load + s_waitcnt, ~100 cycles that nothing
// covers at one wave per SIMD).  ERPL_PIN_SCALARS keeps the hottest in vector registers (in practice in
// the accumulation half: one v_accvgpr_read per dword and use); ERPL_LDS_SCALARS keeps all of them in LDS
// and reads them where they are used (one broadcast ds_read per two constants).
#ifndef ERPL_LDS_SCALARS
#define ERPL_LDS_SCALARS 0
#endif
#ifndef ERPL_PIN_SCALARS
#define ERPL_PIN_SCALARS (ERPL_FAST_F64 && !ERPL_LDS_SCALARS && !ERPL_TWO_WAVE)   // two waves: no registers to pin into
#endif
// Two waves per SIMD for the fp64 throughput build (round 3).  With ONE resident wave every instruction of any
// kind - scalar moves, accumulation-register copies, waits - takes a full issue slot of the SIMD (one slot per
// four cycles); with two, the scalar / LDS / branch instructions of one wave issue beside the vector
// instructions of the other and LDS latency is covered.  Two waves need <= 256 registers per lane, which the
// all-in-registers layout misses by ~100 doubles, so this build keeps in LDS what is touched only at known
// points of a step:
//   ERPL_LDS_Y     the 14-state y of the lane (read when a stage vector is formed, written once per step);
//   ERPL_LDS_WIND  the lane's current wind interval (9 values, read at the top of every RHS evaluation);
//   ERPL_TABLE_IDX the lane keeps only the INDEX of its Mach interval and atmosphere layer and reads the
//                  records from the workgroup's shared LDS tables where the RHS consumes them (a broadcast
//                  when the lanes agree, which they mostly do).
// 64-thread workgroups (one wave), eight of them per CU: 14 + 9 doubles per lane = 11.8 KB plus 4.1 KB of tables
// plus the wind altitude grid (dynamic: K doubles) per workgroup, 132 KB of the CU's 160 KB at K = 100.
#ifndef ERPL_LDS_Y
#define ERPL_LDS_Y ERPL_TWO_WAVE
#endif
#ifndef ERPL_LDS_WIND
#define ERPL_LDS_WIND ERPL_TWO_WAVE
#endif
#ifndef ERPL_TABLE_IDX
#define ERPL_TABLE_IDX ERPL_TWO_WAVE
#endif
#define ERPL_LANE_LDS (ERPL_LDS_Y || ERPL_LDS_WIND)   // the flight kernel runs 64-thread workgroups with per-lane LDS arrays
// Hand-over of blow-ups to the reference-order kernel (round 4).  The fp64 throughput build reproduces the reference
// to ~1e-9 for as long as the state is of physical size; what it cannot reproduce is WHICH intermediate of the last one
// or two RK4 steps of a diverged sample (SURVEY fact 5: speeds of 1e25 .. 1e120 m/s) overflows to inf and which turns
// NaN - that depends on the exact operation order (x * rsq(x) against sqrt(x), a fused against a separate multiply,
// a ratio against the trig of an atan2), and the reference's outcome depends on it: an infinite altitude ends the flight
// at `z > 100 000` (simulator.py:242), a NaN one runs to max_time (:216) - 81 % of round 3's apogee mismatches
// (profiles/r4_divergence_before.txt).  So a lane whose speed passes ERPL_HANDOFF_SPEED (1e6 m/s) or that is 100 km
// below the ground leaves the RK4 loop after that step, is parked in the context's hand-over queue and finishes in the
// reference-order kernel (erpl_launch_f64_sweep behind the last launch of the batch).  From below that bound no
// intermediate of ONE step comes near the overflow threshold (worst case ~1e180, DESIGN.md section 5), and from above
// it a diverging sample has two steps left on average, 31 at most (profiles/r4_blowup_sizing.json: 99.8 % of the bench
// shard's samples pass it, 0.07 % of all steps are made beyond it).  No flight the model is valid for comes near it.
#ifndef ERPL_HANDOFF
#define ERPL_HANDOFF (ERPL_FAST_F64 && !ERPL_FAITHFUL)
#endif
#ifndef ERPL_HANDOFF_SPEED
#define ERPL_HANDOFF_SPEED 1e6
#endif
#ifndef ERPL_DYN_ALT
#define ERPL_DYN_ALT ERPL_LANE_LDS                    // the wind altitude grid sits in dynamic LDS (K values, not 1024)
#endif
// fp32 throughput build: the atmosphere layer's own bounds are cached next to the combined layer-and-wind range,
// so that a wind-knot crossing inside a layer does not re-read the layer record (altitude_tables_reload)
#ifndef ERPL_ATM_LAYER_BOUNDS
#define ERPL_ATM_LAYER_BOUNDS (!ERPL_FAITHFUL && !ERPL_FAST_F64)
#endif

namespace {

constexpr bool kFaithful = (ERPL_FAITHFUL != 0);
constexpr int kWave = 64;
enum { kIdle = 0, kPhysics = 1, kCoast = 2 };                                  // lane modes
enum { kRecChute = 1, kRecNanSeen = 2, kRecApogee = 4, kRecFresh = 8 };       // record flag bits

// Diagnostic build only (-DERPL_STAMPS=1): s_memtime stamps around segments of one integration step,
// summed per wave in scalar registers and added to counters[8..15] at wave exit.  Never in the
// shipped library (the stamps fence the scheduler); read the SHARES, not the run time.
#ifndef ERPL_STAMPS
#define ERPL_STAMPS 0
#endif
#if ERPL_STAMPS
#define ERPL_STAMP(acc_, last_)                                                          \
  do {                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    unsigned long long now_;                                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");          \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    acc_ += now_ - last_;                                                                \
    last_ = now_;                                                                        \
  } while (0)
#else
#define ERPL_STAMP(acc_, last_) do { } while (0)
#endif
struct StampSums { unsigned long long seg[8]; unsigned long long last; };
// Inside a rarely taken block: keeps it a real (wave-skipped) branch instead of being if-converted to
// v_cndmask selects that every step would pay for.
#define ERPL_RARE_BLOCK() asm volatile("")

// ------------------------------------------------------------------------------------ math
__device__ __forceinline__ double m_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ double m_exp(double x) { return exp(x); }
__device__ __forceinline__ double m_pow(double x, double y) { return pow(x, y); }
__device__ __forceinline__ double m_atan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ double m_sin(double x) { return sin(x); }
__device__ __forceinline__ double m_cos(double x) { return cos(x); }
__device__ __forceinline__ double m_abs(double x) { return fabs(x); }
__device__ __forceinline__ double m_div(double a, double b) { return a / b; }
// The polynomial coefficients of the fp64 throughput build's exp2 / log2 / atan.  Left to itself the compiler
// hoists every 64-bit coefficient out of the RK4 loop into VECTOR registers - ~50 doubles that it then spills to
// scratch and re-loads, or copies (v_mov_b64) before each accumulating v_fmac - the opposite of what a
// register-capped loop needs; materialised in scalar registers at their use (two s_mov each) they cost ~100
// scalar instructions per RHS evaluation, and with two waves per SIMD a wave still issues one instruction of ANY
// kind per slot (tools/ubench/f64_issue.hip).  So the coefficients sit in constant memory, one table per
// polynomial, and reach scalar registers by s_load_dwordx8 / x16 behind a laundered pointer (the loads cannot
// leave the loop); a Horner step is then one three-address v_fma_f64 with a scalar addend.
#ifndef ERPL_POLY_TABLES
#define ERPL_POLY_TABLES (ERPL_FAST_F64 && ERPL_TWO_WAVE)
#endif
#if ERPL_POLY_TABLES
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
#define KS(i_, v_, after_) poly_coef(pc[i_], after_)
#elif ERPL_FAST_F64 && ERPL_TWO_WAVE
// A/B build (-DERPL_POLY_TABLES=0): every coefficient materialised in a scalar register pair at its use (two s_mov)
__device__ __forceinline__ double poly_lit(double c) { asm volatile("" : "+s"(c)); return c; }
#define ERPL_POLY(name_, arg_) do { } while (0)
#define KS(i_, v_, after_) poly_lit(v_)
#else
#define ERPL_POLY(name_, arg_) do { } while (0)
#define KS(i_, v_, after_) (v_)
#endif
#if ERPL_FAST_F64
// v_rcp_f64 seed (measured on MI355X: 4.6e-8 relative, tools/ubench/f64_seed.hip) + ONE cubic round
// r (1 + e + e^2), e = 1 - a r: error e^3 ~ 1e-22, result within 1.0 ulp - the same as the two Newton rounds
// of round 2 at three FMAs instead of four.  No denormal / overflow scaling: fast-path operands are
// O(1e-6 .. 1e12); blow-ups go to inf/NaN as in the reference
__device__ __forceinline__ double m_rcp(double a) {
  const double r = __builtin_amdgcn_rcp(a);
  const double e = __builtin_fma(-a, r, 1.0);
  return __builtin_fma(r, __builtin_fma(e, e, e), r);
}
#else
__device__ __forceinline__ double m_rcp(double a) { return 1.0 / a; }
#endif

#if ERPL_FAST_F32
// Hardware transcendental instructions (1 ulp v_rcp/v_sqrt/v_rsq/v_exp/v_log), no denormal or
// range fix-up code.  Inputs on this path are O(1e-6 .. 1e8); blow-ups go to inf/NaN as in fp64.
__device__ __forceinline__ float m_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float m_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float m_pow(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }
__device__ __forceinline__ float m_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float m_rcp(float a) { return __builtin_amdgcn_rcpf(a); }
// atan2 for finite, not-both-zero arguments: octant reduction + odd minimax polynomial on [0,1]
// (max error 1.0e-7 rad), NaN-propagating.
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
  r = (mx != mx || mn != mn) ? (x + y) : r;  // NaN in -> NaN out (fmax/fmin drop NaNs)
  return copysignf(r, y);
}
// Aerodynamic angles of the fast RHS through the half angle: with r = sqrt(x^2 + y^2) supplied by the
// caller (floored > 0, so atan2(0, 0) = 0: the dead zone of utils.py:160-172),
//   atan2(y, |x|) = 2 atan(y / (r + |x|)),  |y / (r + |x|)| <= 1,
// so the [0,1] polynomial applies without octant reduction (no min/max, no pi/2 fix-up) and the sign
// of y comes with the quotient.  Arguments are finite (q_dynamic > 0 has been tested).  XPOS: x >= 0.
// Coefficients are twice those of m_atan2 (max error 2e-7 rad).
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
#else
__device__ __forceinline__ float m_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ float m_exp(float x) { return expf(x); }
__device__ __forceinline__ float m_pow(float x, float y) { return powf(x, y); }
__device__ __forceinline__ float m_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ float m_div(float a, float b) { return a / b; }
__device__ __forceinline__ float m_rcp(float a) { return 1.0f / a; }
#endif
__device__ __forceinline__ float m_sin(float x) { return sinf(x); }
__device__ __forceinline__ float m_cos(float x) { return cosf(x); }
__device__ __forceinline__ float m_abs(float x) { return fabsf(x); }
// min / max / copysign in the working precision (NaN handling of fmin/fmax: the non-NaN operand)
__device__ __forceinline__ float m_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double m_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float m_copysign(float a, float b) { return copysignf(a, b); }
__device__ __forceinline__ double m_copysign(double a, double b) { return copysign(a, b); }
// smallest value above a positive finite x (half-open ranges over closed layer bounds)
__device__ __forceinline__ float m_next_up(float x) { return __int_as_float(__float_as_int(x) + 1); }
__device__ __forceinline__ double m_next_up(double x) { return __longlong_as_double(__double_as_longlong(x) + 1); }

template <typename T> __device__ __forceinline__ bool m_isnan(T x) { return x != x; }

constexpr real kBig = (real)1e30;  // clamp for table abscissae so that 0-slope * inf stays finite

// ------------------------------------------------------------------------------------ cold kernel arguments
// Both kernels take (ErplKArgs a, ErplScalars<real> S) by value.  Only the hot scalars of S (and a
// few ints/doubles) should live in SGPRs across the integration loop; buffer pointers and sizes that
// are needed only when a lane is refilled, finishes, or reloads a table interval are read from the
// kernel-argument segment AT THE POINT OF USE through this laundered pointer (scalar loads, scalar
// cache), so the compiler cannot hoist them out of the loop and spill them into VGPR lanes.
typedef const ErplKArgs __attribute__((address_space(4))) * ColdArgs;
__device__ __forceinline__ ColdArgs cold_args() {
  ColdArgs p = (ColdArgs)__builtin_amdgcn_kernarg_segment_ptr();  // ErplKArgs is the first argument
  asm volatile("" : "+s"(p));
  return p;
}

// ------------------------------------------------------------------------------------ LDS tables
#if ERPL_TABLE_IDX
// record of one Mach interval as the lane reads it by index: lo hi + the 8 np.interp values; one more record
// behind the table is the empty interval (lo > hi) a lane without a cached interval points at
constexpr int kMachRec = ERPL_MACH_REC + 2;
constexpr int kMachRecs = ERPL_MAX_UNION_KNOTS + 2;
constexpr int kMachEmpty = ERPL_MAX_UNION_KNOTS + 1;
#else
constexpr int kMachRec = ERPL_MACH_REC;
constexpr int kMachRecs = ERPL_MAX_UNION_KNOTS + 1;
#endif
struct LdsTables {
  alignas(16) real mach_rec[kMachRecs * kMachRec];
  alignas(16) real atm[ERPL_ATM_LAYERS * ERPL_ATM_REC];
  real union_knots[ERPL_MAX_UNION_KNOTS];
  real curve_t[ERPL_MAX_CURVE_KNOTS];
  real curve_f[ERPL_MAX_CURVE_KNOTS];
  real alt_map[2];   // first knot and knots per metre of the straight line through the end knots (wind_reload's guess)
#if ERPL_LDS_SCALARS
  ErplScalars<real> scalars;   // the uniform constants (fp64 builds: see the flight kernel)
#endif
};

// `alt` = the workgroup's copy of the wind altitude grid (static, or dynamic LDS of k_wind values)
__device__ __forceinline__ void stage_tables(LdsTables& L, real* alt, const ErplTables* __restrict__ T,
                                             const double* __restrict__ alt_grid, int k_wind) {
  const int tid = threadIdx.x, nt = blockDim.x;
#if ERPL_TABLE_IDX
  {
    const int n_union = T->n_union;
    for (int i = tid; i < kMachRecs * kMachRec; i += nt) {
      const int idx = i / kMachRec, k = i - idx * kMachRec;
      real v;
      if (idx > n_union) v = (k == 0) ? (real)1 : (real)0;   // empty interval, zero record
      else if (k == 0) v = (idx == 0) ? (real)-INFINITY : (real)T->union_knots[idx - 1];
      else if (k == 1) v = (idx == n_union) ? (real)INFINITY : (real)T->union_knots[idx];
      else v = (real)T->mach_rec[idx * ERPL_MACH_REC + (k - 2)];
      L.mach_rec[i] = v;
    }
  }
#else
  for (int i = tid; i < (ERPL_MAX_UNION_KNOTS + 1) * ERPL_MACH_REC; i += nt) L.mach_rec[i] = (real)T->mach_rec[i];
#endif
  for (int i = tid; i < ERPL_MAX_UNION_KNOTS; i += nt) L.union_knots[i] = (real)T->union_knots[i];
  for (int i = tid; i < ERPL_MAX_CURVE_KNOTS; i += nt) {
    L.curve_t[i] = (real)T->curve_t[i];
    L.curve_f[i] = (real)T->curve_f[i];
  }
  for (int i = tid; i < k_wind; i += nt) alt[i] = (real)alt_grid[i];
  if (tid == 0) {
    const real a0 = (k_wind > 0) ? (real)alt_grid[0] : (real)0;
    const real span = (k_wind > 1) ? (real)alt_grid[k_wind - 1] - a0 : (real)0;
    L.alt_map[0] = a0;
    L.alt_map[1] = (span > 0) ? (real)(k_wind - 1) / span : (real)0;
  }
  for (int i = tid; i < ERPL_ATM_LAYERS * ERPL_ATM_REC; i += nt) L.atm[i] = (real)T->atm_rec[i];
  __syncthreads();
}

#if ERPL_LDS_SCALARS
// Copy of the by-value kernel argument in LDS (before the barrier of stage_tables is enough: call first).
__device__ __forceinline__ void stage_scalars(LdsTables& L, const ErplScalars<real>& S) {
  constexpr int kWords = (int)(sizeof(ErplScalars<real>) / sizeof(real));
  const real* __restrict__ src = (const real*)&S;
  real* dst = (real*)&L.scalars;
  for (int i = threadIdx.x; i < kWords; i += blockDim.x) dst[i] = src[i];
}
#endif

// ------------------------------------------------------------------------------------ per-lane data
struct LaneParams {
  real dry, prop;             // rocket.dry_mass, rocket.propellant_mass (monte_carlo.py:315-316)
  real thrust, Ae, mdot;      // motor row: thrust_vacuum | curve multiplier, exit area, mass flow
  double burn;                // motor.burn_time, kept fp64 for the t <= burn_time gates
  real dry_cg;                // dry * center_of_mass_dry             (fast path)
  real pfr0, inv_abs_pfr;     // -mdot/prop and 1/|mdot/prop|         (fast path)
};

__device__ __forceinline__ void lane_params_finish(const ErplScalars<real>& S, LaneParams& p) {
  p.dry_cg = p.dry * S.cg_dry;
  p.pfr0 = -p.mdot / p.prop;
  p.inv_abs_pfr = (p.pfr0 != 0) ? (real)1 / ((p.pfr0 < 0) ? -p.pfr0 : p.pfr0) : (real)INFINITY;
}

// Current wind interval of this lane: value = s*(h - x0) + y0 for lo <= h < hi (np.interp,
// environment.py:267-276 / utils.py:147-149).  Reloaded only when the altitude leaves it.
struct WindCache {
  real lo, hi, x0;
  real y0[3], s[3];
};

struct Shared {            // uniform context kept live across the integration loop
  const ErplScalars<real>* S;   // points at the by-value kernel argument (kernarg -> SGPRs)
  const LdsTables* L;
  const real* alt;              // the workgroup's wind altitude grid in LDS
  bool has_wind;
  int motor_kind;
};

__device__ __forceinline__ void wind_reload(const Shared& C, int64_t id, real h, WindCache& wc) {
  const LdsTables& L = *C.L;
  ColdArgs ca = cold_args();
  const int k_wind = ca->k_wind;
  const real* __restrict__ wind = (const real*)ca->wind;
  // j = number of knots <= h (0 for NaN).  The reference's profiles are (near-)uniform grids: guess j from the
  // straight line through the end knots and check it against the two knots around it - two independent LDS
  // reads instead of log2(K) dependent ones; any grid the guess is wrong for takes the bisection.
  const real g = (h - L.alt_map[0]) * L.alt_map[1];
  int j = (g >= 0) ? ((g < (real)k_wind) ? (int)g + 1 : k_wind) : 0;
  real below = (j > 0) ? C.alt[j - 1] : -INFINITY;
  real above = (j < k_wind) ? C.alt[j] : INFINITY;
  if (!(below <= h && h < above)) {
    int lo = 0, hi = k_wind;
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      if (C.alt[mid] <= h) lo = mid + 1; else hi = mid;
    }
    j = lo;
    below = (j > 0) ? C.alt[j - 1] : -INFINITY;
    above = (j < k_wind) ? C.alt[j] : INFINITY;
  }
  const int64_t n = ca->n;
  if (j == 0 || j == k_wind) {
    const int k = (j == 0) ? 0 : k_wind - 1;
    wc.x0 = (j == 0) ? above : below;
    wc.lo = (j == 0) ? -INFINITY : wc.x0;
    wc.hi = (j == 0) ? wc.x0 : INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) { wc.y0[c] = wind[(int64_t)(k * 3 + c) * n + id]; wc.s[c] = 0; }
  } else {
    const real x0 = below, x1 = above;
    wc.x0 = x0; wc.lo = x0; wc.hi = x1;
    const real dx = x1 - x0;
    real v[6];
    // six rows of the table, n elements apart, through one running pointer: all six loads go out before the
    // first is needed (with an address pair per load the register-capped build waited for each knot pair
    // before it issued the next: three memory round trips per reload instead of one)
    const real* __restrict__ row = wind + ((int64_t)(j - 1) * 3 * n + id);
#pragma unroll
    for (int c = 0; c < 6; ++c) { v[c] = *row; row += n; }
#pragma unroll
    for (int c = 0; c < 6; ++c) asm volatile("" : "+v"(v[c]));   // keep the loads ahead of the divisions
#if ERPL_FAITHFUL
#pragma unroll
    for (int c = 0; c < 3; ++c) { wc.y0[c] = v[c]; wc.s[c] = (v[3 + c] - v[c]) / dx; }   // numpy's arr_interp slope
#else
    // throughput builds: one reciprocal for the three slopes (a wave takes this path every other RK4 step at
    // K = 100, and the kernel is issue-bound: three IEEE divisions are 33 instructions)
    const real rdx = m_rcp(dx);
#pragma unroll
    for (int c = 0; c < 3; ++c) { wc.y0[c] = v[c]; wc.s[c] = (v[3 + c] - v[c]) * rdx; }
#endif
  }
}

__device__ __forceinline__ void wind_at(const Shared& C, int64_t id, real h, WindCache& wc, real (&w)[3]) {
  if (!C.has_wind) { w[0] = w[1] = w[2] = 0; return; }
  if (!(h >= wc.lo && h < wc.hi)) wind_reload(C, id, h, wc);
  // (both sides: np.interp gives the end knots' values at +-inf, and 0-slope * (+-inf) would be NaN here.  Round 4: the
  // missing lower clamp made the wind NaN at z = -inf, and with it the parachute branch of 13 of 60 000 blown-up
  // samples end differently from the reference - profiles/r4_gate_vs_oracle_before.txt.)  NaN stays NaN, as in np.interp.
  const real hq = (h > kBig) ? kBig : ((h < -kBig) ? -kBig : h);
  const real d = hq - wc.x0;
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c] = wc.s[c] * d + wc.y0[c];
}

// environment.py:26-103 ; returns temperature, pressure (density = P/(R T) by the caller)
__device__ __forceinline__ void atmosphere(const ErplScalars<real>& S, real h, real& T, real& P) {
  if (h <= S.h_tropo) {
    T = S.T0 - S.lapse * h;
    P = S.P0 * m_pow(m_div(T, S.T0), S.tropo_exp);
  } else if (h <= S.h_strat) {
    T = S.T_strat;
    P = S.p11 * m_exp(m_div(-S.g0 * (h - S.h_tropo), S.Rg * T));
  } else if (h <= (real)32000.0) {
    T = S.T_strat + (real)0.001 * (h - S.h_strat);
    T = ((real)228.65 < T) ? (real)228.65 : T;
    if (h <= (real)25000.0) {
      P = S.p20 * m_exp(m_div(-S.g0 * (h - S.h_strat), S.Rg * S.T_strat));
    } else {
      P = S.p25 * m_pow(m_div(T, S.T_strat), S.grad_exp);
    }
  } else {
    T = (real)228.65 - (real)0.0028 * (h - (real)32000.0);
    T = ((real)180.0 > T) ? (real)180.0 : T;
    const real scale_height = m_div(S.Rg * T, S.g0);
    P = (real)868.02 * m_exp(m_div(-(h - (real)32000.0), scale_height));
  }
}

// environment.py:105-108
__device__ __forceinline__ real gravity_at(const ErplScalars<real>& S, real h) {
  const real re = (real)6.371e6;
  const real r = m_div(re, re + h);
  return S.g0 * (r * r);
}

// rocket.py:110-136
__device__ __forceinline__ void mass_props(const ErplScalars<real>& S, const LaneParams& p, real pf,
                                           real& mass, real& cg, real& Ixx, real& Iyy) {
  const real mp = p.prop * pf;
  mass = p.dry + mp;
  cg = m_div(p.dry * S.cg_dry + mp * S.prop_cg, mass);
  Ixx = S.Ixx_dry + mp * S.dq2;
  const real d = S.prop_cg - cg;
  Iyy = S.Iyy_dry + mp * (S.third + d * d);
}

// Current Mach interval of this lane (union of the Cd and CP-shift knots): the np.interp records
// of rocket.py:156-157 and :107 for lo <= mach < hi.  Reloaded from LDS only when the Mach number
// leaves the interval (a NaN Mach always misses and lands on record 0, whose zero slopes
// propagate the NaN exactly like np.interp does).
#if ERPL_TABLE_IDX
struct MachCache {
  int idx;   // number of union knots <= the Mach numbers of the interval; the record is read from the shared table
};
__device__ __forceinline__ void mach_cache_clear(MachCache& mc) { mc.idx = kMachEmpty; }
__device__ __forceinline__ const real* mach_rec_of(const Shared& C, const MachCache& mc) { return &C.L->mach_rec[mc.idx * kMachRec + 2]; }
__device__ __forceinline__ bool mach_inside(const Shared& C, const MachCache& mc, real mach) {
  const real* r = &C.L->mach_rec[mc.idx * kMachRec];
  const real lo = r[0], hi = r[1];   // one 16-byte read, no short-circuit branch between the two
  return (mach >= lo) & (mach < hi);
}
__device__ __forceinline__ void mach_reload(const Shared& C, real mach, MachCache& mc) {
  const LdsTables& L = *C.L;
  const int n_union = cold_args()->n_union;
  // neighbour on the side the old interval was left, else count the knots (see the register variant below)
  int idx = mc.idx + ((mach >= L.mach_rec[mc.idx * kMachRec + 1]) ? 1 : -1);
  idx = (idx < 0) ? 0 : ((idx > n_union) ? n_union : idx);
  if (!(mach >= L.mach_rec[idx * kMachRec] && mach < L.mach_rec[idx * kMachRec + 1])) {
    idx = 0;
    for (int j = 0; j < n_union; ++j) idx += (mach >= L.union_knots[j]) ? 1 : 0;
  }
  mc.idx = idx;
}
#else
struct MachCache {
  real lo, hi;
  real rec[ERPL_MACH_REC];
  int idx;   // number of union knots <= the Mach numbers of [lo, hi): only a starting guess for the next reload
};
__device__ __forceinline__ void mach_cache_clear(MachCache& mc) {
  mc.lo = 1; mc.hi = 0; mc.idx = 0;
#pragma unroll
  for (int k = 0; k < ERPL_MACH_REC; ++k) mc.rec[k] = 0;
}
__device__ __forceinline__ const real* mach_rec_of(const Shared&, const MachCache& mc) { return mc.rec; }
__device__ __forceinline__ bool mach_inside(const Shared&, const MachCache& mc, real mach) { return mach >= mc.lo && mach < mc.hi; }

__device__ __forceinline__ void mach_reload(const Shared& C, real mach, MachCache& mc) {
  const LdsTables& L = *C.L;
  const int n_union = cold_args()->n_union;
  // idx = number of union knots <= mach (0 for NaN).  Mach moves through the table one interval at a time: try the
  // neighbour on the side the old interval was left (two LDS reads), count the knots only if that is not it.
  int idx = mc.idx + ((mach >= mc.hi) ? 1 : -1);
  idx = (idx < 0) ? 0 : ((idx > n_union) ? n_union : idx);   // (also keeps a guess from an empty cache inside the table)
  real lo = (idx == 0) ? -INFINITY : L.union_knots[idx - 1];
  real hi = (idx == n_union) ? INFINITY : L.union_knots[idx];
  if (!(mach >= lo && mach < hi)) {
    idx = 0;
    for (int j = 0; j < n_union; ++j) idx += (mach >= L.union_knots[j]) ? 1 : 0;
    lo = (idx == 0) ? -INFINITY : L.union_knots[idx - 1];
    hi = (idx == n_union) ? INFINITY : L.union_knots[idx];
  }
  mc.lo = lo; mc.hi = hi; mc.idx = idx;
#pragma unroll
  for (int k = 0; k < ERPL_MACH_REC; ++k) mc.rec[k] = L.mach_rec[idx * ERPL_MACH_REC + k];
}
#endif

__device__ __forceinline__ void mach_lookup(const Shared& C, real mach, MachCache& mc) {
  if (!mach_inside(C, mc, mach)) mach_reload(C, mach, mc);
}

// motor.py:54-76 thrust-curve part: np.interp(t, curve_time, curve_thrust * multiplier)
__device__ __forceinline__ real solid_curve(const Shared& C, real tt, real mult) {
  const LdsTables& L = *C.L;
  const int n_curve = cold_args()->n_curve;
  int j = 0;
  for (int k = 0; k < n_curve; ++k) j += (tt >= L.curve_t[k]) ? 1 : 0;
  if (j == 0) return L.curve_f[0] * mult;
  if (j == n_curve) return L.curve_f[n_curve - 1] * mult;
  const real x0 = L.curve_t[j - 1], x1 = L.curve_t[j];
  const real y0 = L.curve_f[j - 1] * mult, y1 = L.curve_f[j] * mult;
  return m_div(y1 - y0, x1 - x0) * (tt - x0) + y0;
}

// ------------------------------------------------------------------------------------ RHS
#if ERPL_FAITHFUL
struct AtmCache { real lo, hi, alo, ahi; };  // unused by the faithful path (analytic piecewise atmosphere)
__device__ __forceinline__ void atm_cache_clear(AtmCache& ac) { ac.lo = 1; ac.hi = 0; ac.alo = 1; ac.ahi = 0; }
struct LaneRec { __device__ __forceinline__ void put_wind(const WindCache&) const {} };
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
// can trip at an RK trial state, SURVEY fact 9).
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
  const bool burning = (pf > 0) && (t <= p.burn);
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
#if ERPL_FAITHFUL
      sincos(alpha, &sa, &ca); sincos(beta, &sb, &cb);   // one argument reduction for both (same values as sin / cos)
#else
      ca = m_cos(alpha); sa = m_sin(alpha); cb = m_cos(beta); sb = m_sin(beta);
#endif
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
#endif  // ERPL_FAITHFUL

#if !ERPL_FAITHFUL
__device__ __forceinline__ float m_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float m_sqrt_pos(float x) { return m_sqrt(x); }
__device__ __forceinline__ float m_exp2(float x, float /*early*/) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float m_log2(float x, float /*early*/) { return __builtin_amdgcn_logf(x); }
#if ERPL_FAST_F64 || ERPL_STATE_F64
// fp64 fast path (ERPL_PREC_F64_FAST): the same short formulation as the fp32 RHS carried in double.
// v_rsq_f64 seeds a Newton iteration like m_rcp above; exp2 / log2 / atan2 are the device library's
// double routines.
__device__ __forceinline__ double m_rsq(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  // y <- y (1 + e/2 + 3 e^2/8), e = 1 - x y^2 : cubic convergence; the hardware seed is good to 5.2e-8, so ONE
  // round lands within 1.24 ulp - exactly where the second round of round 2 left it (tools/ubench/f64_seed.hip)
  const double e = __builtin_fma(-(x * y), y, 1.0);
  return __builtin_fma(y * e, __builtin_fma(0.375, e, 0.5), y);
}
// sqrt of a positive finite value as x rsq(x) (7 instructions; the library routine scales, fixes up and
// classifies: 17).  +inf gives NaN where sqrt gives +inf: both callers feed a state that is past saving.
__device__ __forceinline__ double m_sqrt_pos(double x) { return x * m_rsq(x); }
__device__ __forceinline__ double m_clamp(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }
#if ERPL_OCML_TRANSCENDENTALS
__device__ __forceinline__ double m_exp2(double x, double) { return exp2(x); }
__device__ __forceinline__ double m_log2(double x, double) { return log2(x); }
template <bool XPOS>
__device__ __forceinline__ double m_atan2_half(double y, double x, double r, double) { (void)r; return atan2(y, x); }
#else
// exp2 / log2 / atan for the operand ranges of this RHS, without the special-case ladders of a general
// libm (those cost ~40 % of its instructions, and with one wave per SIMD every instruction is 4 cycles):
// errors <= 2 ulp, NaN in -> NaN out, results overflow / underflow to inf / 0 through v_ldexp_f64.
// 2^x: x = n + f, |f| <= 1/2, 2^f by the degree-13 Taylor polynomial of exp(f ln 2) (next term 4e-18).
__device__ __forceinline__ double m_exp2(double x, double early) {
  ERPL_POLY(exp2, early);
  x = (x < -1100.0) ? -1100.0 : x;   // -inf (pressure at an infinite altitude) -> 0, not inf - inf
  const double n = __builtin_rint(x);
  const double f = x - n;
  double p = KS(0, 1.3691488853904128e-12, f);
  p = __builtin_fma(p, f, KS(1, 2.5678435993488206e-11, p));
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
  q = __builtin_fma(q, z, KS(1, 0.1373995277037108, q));
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
// s_atan.c (valid to 7/16, < 1 ulp).
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
  s1 = __builtin_fma(s1, w, KS(1, 4.97687799461593236017e-02, s1));
  s2 = __builtin_fma(s2, w, KS(7, -5.83357013379057348645e-02, s2));
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
#define ERPL_ATAN_STEP(i1_, v1_, i2_, v2_)                                    \
  {                                                                           \
    const double k1 = KS(i1_, v1_, s1a), k2 = KS(i2_, v2_, s2a);              \
    s1a = __builtin_fma(s1a, wa, k1); s2a = __builtin_fma(s2a, wa, k2);       \
    s1b = __builtin_fma(s1b, wb, k1); s2b = __builtin_fma(s2b, wb, k2);       \
  }
  ERPL_ATAN_STEP(1, 4.97687799461593236017e-02, 7, -5.83357013379057348645e-02)
  ERPL_ATAN_STEP(2, 6.66107313738753120669e-02, 8, -7.69187620504482999495e-02)
  ERPL_ATAN_STEP(3, 9.09088713343650656196e-02, 9, -1.11111104054623557880e-01)
  ERPL_ATAN_STEP(4, 1.42857142725034663711e-01, 10, -1.99999999998764832476e-01)
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
#endif
#endif
template <typename T>
__device__ __forceinline__ void m_aero_angles(T ya, T xa, T ra, T yb, T xb, T rb, T early, T& alpha, T& beta) {
  alpha = m_atan2_half<false>(ya, xa, ra, early);
  beta = m_atan2_half<true>(yb, xb, rb, early);
}
#if ERPL_FAST_F64 && !ERPL_OCML_TRANSCENDENTALS
__device__ __forceinline__ void m_aero_angles(double ya, double xa, double ra, double yb, double xb, double rb, double early,
                                              double& alpha, double& beta) {
  m_atan2_half_pair(ya, xa, ra, yb, xb, rb, early, alpha, beta);
}
#endif

// Altitude-keyed data of this lane (fast path): the atmosphere layer record (environment.py:26-103 as
// one formula, see erpl_tables.h) and, through [lo, hi), the range of altitudes over which BOTH this
// record and the cached wind interval are valid - one range test per evaluation covers both tables;
// the reload (layer crossing or wind-knot crossing) is rare and reads LDS / HBM.
struct AtmCache {
  real lo, hi;     // altitudes over which BOTH the layer record and the cached wind interval hold
  real alo, ahi;   // altitudes of the layer alone: a wind-knot crossing inside it leaves the record as it is
#if ERPL_TABLE_IDX
  int li;          // layer index: the record is read from the workgroup's table where it is used
#else
  real r[10];  // aT bT Tlo Thi invTref eL href eH eM base
#endif
};
__device__ __forceinline__ void atm_cache_clear(AtmCache& ac) {
  ac.lo = 1; ac.hi = 0; ac.alo = 1; ac.ahi = 0;
#if ERPL_TABLE_IDX
  ac.li = 0;
#endif
}

__device__ __forceinline__ void altitude_tables_reload(const Shared& C, int64_t id, real h, WindCache& wc, AtmCache& ac) {
  const ErplScalars<real>& S = *C.S;
  // (fp32 build only: in the fp64 build the two extra doubles cost more in accumulation-register copies than the
  // skipped record load saves - measured)
  if (!ERPL_ATM_LAYER_BOUNDS || !(h >= ac.alo && h < ac.ahi)) {   // layer crossing (or nothing cached yet, or NaN): four times per flight
    const int li = ((h > S.h_tropo) ? 1 : 0) + ((h > S.h_strat) ? 1 : 0) + ((h > (real)25000.0) ? 1 : 0) +
                   ((h > (real)32000.0) ? 1 : 0);  // NaN -> layer 0, whose formula propagates the NaN
#if ERPL_TABLE_IDX
    ac.li = li;
#else
#pragma unroll
    for (int k = 0; k < 10; ++k) ac.r[k] = C.L->atm[li * ERPL_ATM_REC + k];
#endif
    // layer li covers (llo, lhi]; as a half-open float range: [next(llo), next(lhi))
    const real llo = (li == 0) ? -INFINITY : ((li == 1) ? S.h_tropo : ((li == 2) ? S.h_strat : ((li == 3) ? (real)25000.0 : (real)32000.0)));
    const real lhi = (li == 0) ? S.h_tropo : ((li == 1) ? S.h_strat : ((li == 2) ? (real)25000.0 : ((li == 3) ? (real)32000.0 : INFINITY)));
    ac.alo = (llo > -INFINITY) ? m_next_up(llo) : llo;  // bounds are positive finite values
    ac.ahi = (lhi < INFINITY) ? m_next_up(lhi) : lhi;
  }
  real lo = ac.alo, hi = ac.ahi;
  if (C.has_wind) {
    if (!(h >= wc.lo && h < wc.hi)) wind_reload(C, id, h, wc);
    lo = (wc.lo > lo) ? wc.lo : lo;
    hi = (wc.hi < hi) ? wc.hi : hi;
  }
  ac.lo = lo; ac.hi = hi;
}

// Handle of the lane's LDS-resident data for the RHS (ERPL_LDS_WIND): the wind interval is loaded right where the
// RHS consumes it (behind a compiler-level memory fence, so that the loads are not hoisted and held in registers
// through the evaluation); in the register builds the handle is empty and the calls vanish.  Layout: value k of
// lane l at lw[k * 64 + l] (conflict-free 8-byte reads).
enum { kLwLo = 0, kLwHi, kLwX0, kLwY0, kLwS = kLwY0 + 3, kLwSlots = kLwS + 3 };
struct LaneRec {
#if ERPL_LDS_WIND
  real* lw;
  __device__ __forceinline__ void fence() const { asm volatile("" ::: "memory"); }
  __device__ __forceinline__ void wind_bounds(WindCache& wc) const { wc.lo = lw[kLwLo * kWave]; wc.hi = lw[kLwHi * kWave]; }
  __device__ __forceinline__ void wind(WindCache& wc) const {
    wc.x0 = lw[kLwX0 * kWave];
#pragma unroll
    for (int c = 0; c < 3; ++c) { wc.y0[c] = lw[(kLwY0 + c) * kWave]; wc.s[c] = lw[(kLwS + c) * kWave]; }
  }
  __device__ __forceinline__ void put_wind(const WindCache& wc) const {
    lw[kLwLo * kWave] = wc.lo; lw[kLwHi * kWave] = wc.hi; lw[kLwX0 * kWave] = wc.x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { lw[(kLwY0 + c) * kWave] = wc.y0[c]; lw[(kLwS + c) * kWave] = wc.s[c]; }
  }
#else
  __device__ __forceinline__ void fence() const {}
  __device__ __forceinline__ void wind_bounds(WindCache&) const {}
  __device__ __forceinline__ void wind(WindCache&) const {}
  __device__ __forceinline__ void put_wind(const WindCache&) const {}
#endif
};

// environment.py:26-103 through the lane's layer record (erpl_tables.h): temperature, its reciprocal
// and pressure.
__device__ __forceinline__ void fast_atmosphere(const Shared& C, const AtmCache& ac, real h, real& T, real& rT, real& P) {
#if ERPL_TABLE_IDX
  const real* r = &C.L->atm[ac.li * ERPL_ATM_REC];
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
    cl = cl_alpha * m_copysign(m_clamp(abs_alpha, (real)-1, S.stall_angle) * sf, alpha);  // min(|alpha|, stall)
  }
  const real sm = (S.cp_location + cps) - cg;
  cma = -cl_alpha * sm;
}

// Fast RHS: the same equations as the faithful rocket_dynamics() (simulator.py:295-460) with
// algebraically identical shortcuts (one reciprocal per denominator, rsq for 1/sqrt, cos/sin(atan2)
// as ratios, croll == 0 and Izz == Iyy used explicitly, the atmosphere layers as one exp2/log2 formula
// over a per-layer coefficient record).  The vector-ALU issue port is the resource this kernel runs
// out of (DESIGN.md section 3), so the code is written for a short instruction stream: the
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
  const bool burning = (pf > 0) && (GATED ? gate_le_burn : (t <= p.burn));
  real thrust;
  if (C.motor_kind == ERPL_MOTOR_SOLID) {  // wave-uniform
    thrust = burning ? solid_curve(C, GATED ? gate_t : (real)t, p.thrust) + p.Ae * ((real)101325.0 - P) : (real)0;
  } else {
    thrust = burning ? p.thrust - p.Ae * P : (real)0;
  }
  real fb0 = thrust, fb1 = 0, fb2 = 0, mb1 = 0, mb2 = 0;
  ERPL_STAMP(ss.seg[2], ss.last);
  // ---- parachute latch (:366-369) and drag (:372-377) ----
  // A wave-skipped branch, not selects: the parachute is out in <1 % of all evaluations, and on this
  // kernel the vector-ALU port is the saturated resource (tools/ubench/valu_issue.hip: v_cmp and
  // v_cndmask cost ~4.1 cycles each per SIMD vs ~2.7 for an FMA) - measured -5 % time.  The other
  // small conditionals stay predicated: as branches they cost more (phi copies, exec bookkeeping).
  if (h <= S.chute_alt) { if (!chute && y[5] < 0) chute = true; }  // below 500 m only
  if (chute) {
    const real rs2 = (vb0 * vb0 + vb1 * vb1) + vb2 * vb2;
    const real rs = m_sqrt(rs2);
    if (rs > 0) {
      const real rho = (P * S.inv_Rg) * rT;
      const real kc = -(rho * rs2) * S.chute_k * m_rcp(rs);
      fb0 += kc * vb0; fb1 += kc * vb1; fb2 += kc * vb2;
    }
  }
  if (!chute && qdyn > 0) {  // aerodynamics (:378-411, rocket.py:138-218)
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
    fast_aero(S, mach_rec_of(C, mc), mach, mach2, alpha, beta, pf, cg, cd, cl, cy, cma);
    const real qs = qdyn * S.ref_area;
    const real drag = qs * cd, lift = qs * cl, side = qs * cy;
    fb0 += (sb * side - (ca * cb) * drag) - (sa * cb) * lift;
    fb1 += (-(ca * sb) * drag - cb * side) - (sa * sb) * lift;
    fb2 += sa * drag - ca * lift;
    const real qsd = qdyn * S.area_diam;
    mb1 = qsd * (cma * alpha);
    mb2 = qsd * (cma * beta);
  }
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
#endif  // !ERPL_FAITHFUL

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
    state_t* rr = (state_t*)a.res_r[0];
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

// ------------------------------------------------------------------------------------ kernel 2
struct Lane {
#if ERPL_LDS_Y
  state_t* yl;               // the lane's state in LDS: values 2m, 2m+1 adjacent (one 16-byte read), pairs 64 lanes apart
#else
  state_t y[14];
#endif
  double t, t_rail;
  double apogee_t, first_apogee_t, latch_t;
  state_t apogee, first_apogee;
  real max_speed2, max_coast;
  real cx, cy;               // per-step x/y increments while coasting
  int64_t id;
  int64_t traj_slot;
  int32_t steps, nrail;
  int32_t mode;
  int32_t stop_steps;        // step count at which this launch parks the lane (chunking)
  bool chute, nan_seen, apogee_detected;
};

#if ERPL_LDS_Y
#define LY(ln_, c_) (ln_).yl[((c_) >> 1) * (2 * kWave) + ((c_) & 1)]
#else
#define LY(ln_, c_) (ln_).y[c_]
#endif

template <bool TRAJ>
__device__ __forceinline__ void traj_record(Lane& ln, int64_t& traj_len, bool final) {
  if (!TRAJ) return;
  if (ln.traj_slot < 0) return;
  ColdArgs a = cold_args();
  if (!(final || (a->traj_stride > 0 && (ln.steps % a->traj_stride) == 0))) return;
  int64_t slot = traj_len;
  const int64_t cap = a->traj_cap;
  if (slot >= cap) { if (!final) return; slot = cap - 1; } else traj_len++;
  double* o = a->traj + (ln.traj_slot * cap + slot) * ERPL_TRAJ_DIM;
  o[0] = ln.t;
#pragma unroll
  for (int c = 0; c < 14; ++c) o[1 + c] = (double)LY(ln, c);
}

__device__ __forceinline__ void lane_finish(Lane& ln, int end) {
  ColdArgs a = cold_args();
  const int64_t n = a->n, i = ln.id;
  if (!ln.apogee_detected) { ln.first_apogee = ln.apogee; ln.first_apogee_t = ln.apogee_t; }
  double* s = a->summary;
  const double x = (double)LY(ln, 0), yv = (double)LY(ln, 1);
  s[ERPL_SUM_APOGEE_ALT * n + i] = (double)ln.apogee;
  s[ERPL_SUM_APOGEE_TIME * n + i] = ln.apogee_t - ln.t_rail;
  s[ERPL_SUM_FIRST_APOGEE_ALT * n + i] = (double)ln.first_apogee;
  s[ERPL_SUM_FIRST_APOGEE_TIME * n + i] = ln.first_apogee_t - ln.t_rail;
  s[ERPL_SUM_RANGE * n + i] = sqrt(x * x + yv * yv);
  s[ERPL_SUM_FLIGHT_TIME * n + i] = ln.t - ln.t_rail;
  s[ERPL_SUM_IMPACT_X * n + i] = x;
  s[ERPL_SUM_IMPACT_Y * n + i] = yv;
  s[ERPL_SUM_IMPACT_Z * n + i] = (double)LY(ln, 2);
  s[ERPL_SUM_STEPS * n + i] = (double)ln.steps;
  s[ERPL_SUM_FINAL_VZ * n + i] = (double)LY(ln, 5);
  s[ERPL_SUM_MAX_SPEED * n + i] = (double)m_sqrt(ln.max_speed2);
  a->status[i] = end | (ln.apogee_detected ? ERPL_ST_APOGEE_LATCHED : 0) | (ln.chute ? ERPL_ST_CHUTE : 0) |
                 (ln.nan_seen ? ERPL_ST_NAN : 0);
  ln.mode = kIdle;
}

// One lane's record into a resume queue (the next phase's, or the hand-over queue): entry e of [..][cap] rows.
__device__ __forceinline__ void park_record(Lane& ln, int64_t traj_len, state_t* rr, double* rd, int32_t* ri, int64_t cap,
                                            unsigned long long e) {
#pragma unroll
  for (int c = 0; c < 14; ++c) rr[c * cap + e] = LY(ln, c);
  rr[14 * cap + e] = ln.apogee; rr[15 * cap + e] = ln.first_apogee; rr[16 * cap + e] = ln.max_speed2;
  rr[17 * cap + e] = ln.max_coast; rr[18 * cap + e] = ln.cx; rr[19 * cap + e] = ln.cy;
  rd[0 * cap + e] = ln.t; rd[1 * cap + e] = ln.t_rail; rd[2 * cap + e] = ln.apogee_t;
  rd[3 * cap + e] = ln.first_apogee_t; rd[4 * cap + e] = ln.latch_t;
  ri[0 * cap + e] = (int32_t)ln.id; ri[1 * cap + e] = ln.steps; ri[2 * cap + e] = ln.nrail;
  ri[3 * cap + e] = (ln.mode << 8) | (ln.chute ? kRecChute : 0) | (ln.nan_seen ? kRecNanSeen : 0) |
                    (ln.apogee_detected ? kRecApogee : 0);
  ri[4 * cap + e] = (int32_t)traj_len;
  ln.mode = kIdle;
}

// y += (dt/6) * (k1 + 2 k2 + 2 k3 + k4)  (simulator.py:224); one definition shared by the RK4
// step and the coast fast path so both round identically.
__device__ __forceinline__ state_t rk4_combine(state_t y, state_t dt_sixth, real acc, real k4) {
#if ERPL_STATE_F64
  return y + dt_sixth * ((state_t)acc + (state_t)k4);
#else
  return y + dt_sixth * (acc + k4);
#endif
}

template <typename T> __device__ __forceinline__ bool m_finite(T x) { return (x - x) == (T)0; }

// The register-capped fp32 build keeps the lane's clock (a double) in LDS through the RK4 loop: the compiler
// spilled exactly that pair to scratch and re-read it at every stage, and a scratch load is a vector-memory
// load - it shares the in-order counter with the table reloads, so every stage start waited for whatever
// reload or prefetch was still in flight.  LDS reads come back on the other counter.
#ifndef ERPL_T_IN_LDS
#define ERPL_T_IN_LDS (!ERPL_FAITHFUL && !ERPL_FAST_F64 && !ERPL_STATE_F64 && !ERPL_STEP_COAST)
#endif
#ifndef ERPL_STAGE_UNROLL
#define ERPL_STAGE_UNROLL 1   // 1 = rolled stage loop (one RHS instance), 4 = fully unrolled
#endif
#ifndef ERPL_DENSE_WAVES
#define ERPL_DENSE_WAVES 3      // resident waves per SIMD of the register-capped build used for large batches
#endif
#ifndef ERPL_FLIGHT_MIN_WAVES
#define ERPL_FLIGHT_MIN_WAVES 1   // min waves per SIMD the register allocator must leave room for
#endif
// SPEC >= 0 compiles the two launch-constant switches of the RHS in: bit 0 = a wind table is present,
// bit 1 = solid motor (thrust curve); SPEC < 0 reads them at run time (trajectory-capture build).
// MINW = waves per SIMD the register allocator must leave room for: 1 = all 256 VGPRs (two resident
// waves, no spills: the build for batches that fit two waves per SIMD anyway); 3 = capped at 168 VGPRs,
// three resident waves at the price of ~80 spilled registers - measured +6 % on batches that keep three
// waves per SIMD busy (DESIGN.md section 3).  Same arithmetic, bitwise identical results (tested).
#if ERPL_LANE_LDS
constexpr int kFlightBlock = kWave;   // per-lane LDS arrays of one wave: always 64-thread workgroups
#else
constexpr int kFlightBlock = 256;
#endif
template <bool TRAJ, int SPEC, int MINW>
__global__ __launch_bounds__(kFlightBlock, MINW) void ERPL_CAT(erpl_flight_, ERPL_SUFFIX)(const ErplKArgs a, const ErplScalars<real> S_arg) {
  {  // a launch (or a workgroup) with nothing left in its queue leaves before touching anything
    // (records of this phase that waves of the previous launch already adopted are behind qhead; a
    // stale qhead only lets a workgroup too many start - block 0 never leaves while anything is queued)
    const unsigned long long n_in0 = (a.phase == 0) ? (unsigned long long)a.n : a.qcnt[a.phase];
    const unsigned long long taken0 = (a.phase == 0) ? 0ull : a.qhead[a.phase];
    if ((unsigned long long)blockIdx.x * blockDim.x >= n_in0 - (taken0 < n_in0 ? taken0 : n_in0)) return;
  }
  __shared__ LdsTables L;
#if ERPL_DYN_ALT
  extern __shared__ double erpl_dyn_lds[];            // k_wind values (the launcher sizes it)
  real* const alt_s = (real*)erpl_dyn_lds;
#else
  __shared__ real alt_s[ERPL_MAX_WIND_KNOTS];
#endif
#if ERPL_LDS_SCALARS
  stage_scalars(L, S_arg);
#endif
  stage_tables(L, alt_s, a.tables, a.alt_grid, a.k_wind);
  Shared C;
#if ERPL_LDS_SCALARS
  const ErplScalars<real>& S = L.scalars;
#elif ERPL_PIN_SCALARS
  // fp64 builds run one wave per SIMD and have twice the scalar-register demand (two SGPRs per
  // constant): the compiler re-loads the scalars that do not fit from the kernel-argument segment inside
  // the RK4 loop, every load a ~100-cycle stall nothing else on the SIMD can cover.  Copies of the hot
  // ones pinned in vector registers cost one v_accvgpr_read at worst (the kernel has 512 registers).
  ErplScalars<real> SV = S_arg;
#define ERPL_PIN(f) asm volatile("" : "+v"(SV.f))
  ERPL_PIN(prop_cg); ERPL_PIN(two_pi_AR_cos); ERPL_PIN(AR_over_cos2); ERPL_PIN(stall_angle); ERPL_PIN(inv_stall_span);
  ERPL_PIN(cp_location); ERPL_PIN(ref_area); ERPL_PIN(area_diam); ERPL_PIN(pitch_damping); ERPL_PIN(yaw_damping);
  ERPL_PIN(dt_flight); ERPL_PIN(half_dt); ERPL_PIN(dt_sixth);
#undef ERPL_PIN
  const ErplScalars<real>& S = SV;
#else
  const ErplScalars<real>& S = S_arg;
#endif
  C.S = &S;
  C.L = &L;
  C.alt = alt_s;
  C.has_wind = (SPEC < 0) ? (a.k_wind > 0) : ((SPEC & 1) != 0);
  C.motor_kind = (SPEC < 0) ? a.motor_kind : ((SPEC & 2) ? (int)ERPL_MOTOR_SOLID : (int)ERPL_MOTOR_LIQUID);
  const double dt = a.dt_flight, max_time = a.max_time;
#if ERPL_STATE_F64
  const state_t dt_sixth = dt / 6.0, half_dt = 0.5 * dt, full_dt = dt;
#else
  const state_t dt_sixth = S.dt_sixth, half_dt = S.half_dt, full_dt = S.dt_flight;
#endif
  const int refill_threshold = a.refill_threshold;
  const int chunk_steps = a.chunk_steps;
  const int adopt_lanes = TRAJ ? 0 : a.adopt_lanes;
  const bool stop_at_apogee = (a.flags & ERPL_FLAG_STOP_AT_APOGEE) != 0;
  // capture build: the caller reads time and position of the records only (ERPL_FLAG_CAPTURE_POSITION_ONLY), so a sample
  // whose position is non-finite for good is fast-forwarded like in the plain build - its remaining records carry the exact
  // time stamps and the frozen state - instead of being integrated step by step to max_time (57 000 steps for one wave)
  const bool traj_fast_forward = TRAJ && (a.flags & ERPL_FLAG_CAPTURE_POSITION_ONLY) != 0;
  const int lane = threadIdx.x & (kWave - 1);

  Lane ln;
  ln.mode = kIdle; ln.id = -1; ln.traj_slot = -1;
  LaneParams p;
  WindCache wc;
  MachCache mc;
  mach_cache_clear(mc);
  AtmCache ac;
  atm_cache_clear(ac);
  LaneRec lr;
#if ERPL_LDS_Y
  __shared__ __attribute__((aligned(16))) state_t lane_y[7][kWave][2];
  ln.yl = &lane_y[0][threadIdx.x][0];
#endif
#if ERPL_LDS_WIND
  __shared__ real lane_wind[kLwSlots][kWave];
  lr.lw = &lane_wind[0][threadIdx.x];
#endif
#if ERPL_T_IN_LDS
  __shared__ double t_store[2][256];
  double* const tl = &t_store[0][threadIdx.x];   // the lane's clock while it integrates
  double* const bl = &t_store[1][threadIdx.x];   // and its motor's burn time
#endif
  int64_t traj_len = 0;
  bool queue_empty = false;
  unsigned long long wave_iters = 0, steps_done = 0;
  StampSums ss;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss.seg[i] = 0;
  ss.last = 0;
#if ERPL_STAMPS
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ss.last)::"memory");
#endif

#if ERPL_HANDOFF
  bool extreme = false;
#endif
  for (;;) {
#if ERPL_HANDOFF
    // ---- hand-over: a lane that left the RK4 loop at an unphysical speed goes to the reference-order kernel
    // (ERPL_HANDOFF above); before the chunk / adoption parking below, which would send it round this kernel again ----
    {
      const bool hx = (ln.mode == kPhysics) && extreme;
      const unsigned long long xm = __ballot(hx);
      if (xm != 0ull) {
        ColdArgs ca = cold_args();
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(ca->ext_cnt, (unsigned long long)__popcll(xm));
        base = __shfl(base, 0);
        if (hx) {
          const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(xm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)xm, 0));
          park_record(ln, traj_len, (state_t*)ca->ext_r, ca->ext_d, ca->ext_i, ca->res_cap, base + (unsigned long long)rank);
        }
      }
      extreme = false;
    }
#endif
    // ---- compaction: lanes that used up their step chunk park their state densely in the next
    // phase's queue (one ballot-aggregated atomic per wave) and become idle ----
    {
      // lane adoption: with nothing left to refill from, a wave down to a few flying lanes costs almost
      // what a full one does (DESIGN.md section 3: a half-empty wave issues 87-90 % of a full one's
      // cycles).  It hands those lanes over through the next phase's queue and leaves; waves that still
      // fly more take them into their idle lanes (below), the next launch sweeps up what nobody took.
      bool thin = false;
      if (adopt_lanes > 0 && queue_empty) thin = __popcll(__ballot(ln.mode == kPhysics)) <= adopt_lanes;
      const bool need = (ln.mode == kPhysics) && (thin || ln.steps >= ln.stop_steps);
      const unsigned long long dm = __ballot(need);
      if (dm != 0ull) {
        ColdArgs ca = cold_args();
        const int ph = ca->phase;
        const int64_t cap = ca->res_cap;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&ca->qcnt[ph + 1], (unsigned long long)__popcll(dm));
        base = __shfl(base, 0);
        if (need) {
          const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(dm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)dm, 0));
          const unsigned long long e = base + (unsigned long long)rank;
          park_record(ln, traj_len, (state_t*)ca->res_r[(ph + 1) & 1], ca->res_d[(ph + 1) & 1], ca->res_i[(ph + 1) & 1], cap, e);
        }
        if (adopt_lanes > 0) {
          // publish to waves of THIS launch: records first, then - after a device-scope release - the
          // per-record ready word an adopter spins on before its acquire
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
          if (need) {
            const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(dm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)dm, 0));
            __hip_atomic_store(&ca->res_i[(ph + 1) & 1][5 * cap + (int64_t)(base + (unsigned long long)rank)], ph + 1,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
    // ---- refill idle lanes from the device-wide queue (wave-uniform control flow) ----
    const unsigned long long idle = __ballot(ln.mode == kIdle);
    const int n_idle = __popcll(idle);
    // adoption: the own queue is drained, this wave keeps flying (more lanes than the parking limit) and
    // has room - take records other waves of this launch parked in the next phase's queue.  One
    // compare-and-swap on that queue's pop cursor, never beyond what is reserved there; no waiting
    // except for a record whose writer is between reserving and publishing it.
    const bool adopt = adopt_lanes > 0 && queue_empty && n_idle > 0 &&
                       __popcll(__ballot(ln.mode == kPhysics)) > adopt_lanes;   // (coasting lanes of the fp64 builds do not count)
    if ((!queue_empty && n_idle >= refill_threshold) || adopt) {
      ColdArgs ca = cold_args();
      const int64_t n = ca->n;
      const int ph = ca->phase;
      const int src = adopt ? ph + 1 : ph;
      const int64_t cap = ca->res_cap;
      unsigned long long n_in = (ph == 0) ? (unsigned long long)n : ca->qcnt[ph];
      const state_t* __restrict__ rr = (const state_t*)ca->res_r[src & 1];
      const double* __restrict__ rd = ca->res_d[src & 1];
      const int32_t* __restrict__ ri = ca->res_i[src & 1];
      const double* __restrict__ rocket = ca->rocket;
      const double* __restrict__ motor = ca->motor;
      unsigned long long base = 0;
      if (!adopt) {
        if (lane == 0) base = atomicAdd(&ca->qhead[ph], (unsigned long long)n_idle);
        base = __shfl(base, 0);
        if (base + (unsigned long long)n_idle >= n_in) queue_empty = true;
      } else {
        unsigned long long got = 0;
        if (lane == 0) {
          const unsigned long long r = __hip_atomic_load(&ca->qcnt[src], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          unsigned long long h = __hip_atomic_load(&ca->qhead[src], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (h < r) {
            const unsigned long long want = (r - h < (unsigned long long)n_idle) ? r - h : (unsigned long long)n_idle;
            if (__hip_atomic_compare_exchange_strong(&ca->qhead[src], &h, h + want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) { base = h; got = want; }
          }
        }
        base = __shfl(base, 0);
        n_in = base + __shfl(got, 0);   // nothing claimed: no lane passes e < n_in
      }
      if (ln.mode == kIdle) {
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0));
        const unsigned long long e = base + (unsigned long long)rank;
        if (e < n_in) {
          bool lost = false;
          if (adopt) {
            // the writer is a running wave a few stores away from publishing; the bound only keeps a logic
            // error from hanging the GPU.  A record that never shows up is NOT consumed (its fields may be
            // stale): the lane stays idle, the sample keeps ERPL_ST_INCOMPLETE and counters[3] fails the batch
            // where the host checks it (erpl_mc_check_batch / erpl_mc_synchronize).
            const int limit = ca->adopt_spin;
            int spins = 0;
            lost = limit < 0;
            while (!lost && __hip_atomic_load(&ri[5 * cap + e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != src) {
              __builtin_amdgcn_s_sleep(8);
              if (++spins > limit) lost = true;
            }
            if (lost) atomicAdd(&ca->counters[3], 1ull);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          }
          if (!lost) {
          // ---- load one lane record (fresh from the rail kernel, or dumped by the previous launch) ----
#pragma unroll
          for (int c = 0; c < 14; ++c) LY(ln, c) = rr[c * cap + e];
          ln.apogee = rr[14 * cap + e]; ln.first_apogee = rr[15 * cap + e]; ln.max_speed2 = (real)rr[16 * cap + e];
          ln.max_coast = (real)rr[17 * cap + e]; ln.cx = (real)rr[18 * cap + e]; ln.cy = (real)rr[19 * cap + e];
          ln.t = rd[0 * cap + e]; ln.t_rail = rd[1 * cap + e]; ln.apogee_t = rd[2 * cap + e];
          ln.first_apogee_t = rd[3 * cap + e]; ln.latch_t = rd[4 * cap + e];
          const int64_t id = ri[0 * cap + e];
          ln.id = id; ln.steps = ri[1 * cap + e]; ln.nrail = ri[2 * cap + e];
          const int fl = ri[3 * cap + e];
          ln.mode = fl >> 8;
          ln.chute = (fl & kRecChute) != 0; ln.nan_seen = (fl & kRecNanSeen) != 0;
          ln.apogee_detected = (fl & kRecApogee) != 0;
          ln.stop_steps = (chunk_steps > 0) ? ln.steps + chunk_steps : 0x7fffffff;
          p.dry = (real)rocket[0 * n + id]; p.prop = (real)rocket[1 * n + id];
          p.thrust = (real)motor[0 * n + id]; p.Ae = (real)motor[1 * n + id];
          p.mdot = (real)motor[2 * n + id]; p.burn = motor[3 * n + id];
#if ERPL_T_IN_LDS
          *bl = p.burn;
#endif
          lane_params_finish(S, p);
          wc.lo = 1; wc.hi = 0; wc.x0 = 0;   // table-interval caches start empty: first use reloads
#pragma unroll
          for (int c = 0; c < 3; ++c) { wc.y0[c] = 0; wc.s[c] = 0; }
          lr.put_wind(wc);
          mach_cache_clear(mc);
          atm_cache_clear(ac);
          if (TRAJ) {
            ln.traj_slot = -1; traj_len = ri[4 * cap + e];
            for (int64_t m = 0; m < ca->n_traj; ++m) if (ca->traj_ids[m] == id) ln.traj_slot = m;
          }
          if (fl & kRecFresh) {
            traj_record<TRAJ>(ln, traj_len, false);
            if (!(ln.t < max_time)) {  // while t < max_time never entered
              traj_record<TRAJ>(ln, traj_len, true);
              if (TRAJ && ln.traj_slot >= 0) ca->traj_len[ln.traj_slot] = traj_len;
              lane_finish(ln, ERPL_END_MAX_TIME);
            }
          }
          }  // !lost
        }
      }
    }
    const unsigned long long phys = __ballot(ln.mode == kPhysics);
    if (phys == 0ull) {
      // ---- no lane integrates physics: run the cheap coast lanes in a burst, or leave ----
      if (__ballot(ln.mode == kCoast) == 0ull) { if (queue_empty) break; else continue; }
      for (int burst = 0; burst < 256; ++burst) {
        if (ln.mode == kCoast) {
          LY(ln, 0) = rk4_combine(LY(ln, 0), dt_sixth, ln.cx, (real)0);
          LY(ln, 1) = rk4_combine(LY(ln, 1), dt_sixth, ln.cy, (real)0);
          ln.t += dt;
          ln.steps++;
          if (!(ln.t < max_time)) lane_finish(ln, ERPL_END_MAX_TIME);
        }
        if (__ballot(ln.mode == kCoast) == 0ull) break;
      }
      continue;
    }
    // ---- hot loop: RK4 steps until some lane needs attention (it ended, turned non-finite or used up
    // its step chunk).  A single back-edge with a wave-uniform exit keeps the whole lane state in place
    // in its registers; everything rare - finishing lanes, compaction, refill - happens outside. ----
    bool ended, nonfinite, alt_nan, latch_now, coast_out;
    ERPL_STAMP(ss.seg[0], ss.last);  // refill / ballots
#if ERPL_T_IN_LDS
    if (ln.mode == kPhysics) *tl = ln.t;
#endif
    do {
    ++wave_iters;
    ended = false; nonfinite = false; alt_nan = false; latch_now = false; coast_out = false;
#if ERPL_HANDOFF
    extreme = false;
#endif
    if (ERPL_STEP_COAST && ln.mode == kCoast) {
      // z is NaN, thrust is off: no force has a finite/non-zero horizontal part any more, vx and vy are
      // constant, every comparison of the event logic is false -> only x, y and t advance.
      LY(ln, 0) = rk4_combine(LY(ln, 0), dt_sixth, ln.cx, (real)0);
      LY(ln, 1) = rk4_combine(LY(ln, 1), dt_sixth, ln.cy, (real)0);
      ln.t += dt;
      ln.steps++;
      if (!(ln.t < max_time)) lane_finish(ln, ERPL_END_MAX_TIME);
    }
    if (ln.mode == kPhysics) {
      // ---- one classic RK4 step (:217-229): the four stages run through one instance of the RHS in the reference-order
      // build (rolled stage loop: 4x smaller code, same arithmetic) and through four in the throughput builds
      // (ERPL_STAGE_UNROLL 4) ----
      real k[14], ys[14], acc[14];
#pragma unroll
      for (int c = 0; c < 14; ++c) { ys[c] = (real)LY(ln, c); acc[c] = 0; }
#if !ERPL_FAITHFUL
      // the three stage times of this step against the burn time, and as thrust-curve abscissae: the same fp64
      // sums and comparisons the stages would make, made here so that the stages carry one integer
      int gates;
      real gate_t[3] = {0, 0, 0};
      {
#if ERPL_T_IN_LDS
        const double tb = *tl, burn = *bl;
#else
        const double tb = ln.t, burn = p.burn;
#endif
        const double th = tb + 0.5 * dt, tf = tb + dt;
        gates = ((tb <= burn) ? 1 : 0) | ((th <= burn) ? 2 : 0) | ((tf <= burn) ? 4 : 0);
        if (C.motor_kind == ERPL_MOTOR_SOLID) { gate_t[0] = (real)tb; gate_t[1] = (real)th; gate_t[2] = (real)tf; }
      }
#if ERPL_T_IN_LDS
      asm volatile("" ::: "memory");   // the clock is read again after the stages, not carried through them
#endif
#endif
#pragma unroll ERPL_STAGE_UNROLL
      for (int stage = 0; stage < 4; ++stage) {
#if ERPL_FAITHFUL
        const double ts = (stage == 0) ? ln.t : ((stage == 3) ? ln.t + dt : ln.t + 0.5 * dt);
        rocket_dynamics(C, p, ln.id, wc, mc, ac, ln.chute, ts, ys, k, ss);
#else
        const int gi = (stage == 0) ? 0 : ((stage == 3) ? 2 : 1);
        rocket_dynamics_at<true>(C, p, ln.id, wc, mc, ac, ln.chute, 0.0, ((gates >> gi) & 1) != 0, gate_t[gi], ys, k, ss, lr);
#endif
        const real wgt = (stage == 0 || stage == 3) ? (real)1 : (real)2;   // k1 + 2 k2 + 2 k3 + k4
        const state_t adv = (stage == 2) ? full_dt : half_dt;              // y + dt/2 k1, + dt/2 k2, + dt k3
        if (stage < 3) {
#pragma unroll
          for (int c = 0; c < 14; ++c) {
            acc[c] = (stage == 0) ? k[c] : acc[c] + wgt * k[c];
            ys[c] = (real)(LY(ln, c) + adv * (state_t)k[c]);
          }
        }
        ERPL_STAMP(ss.seg[5], ss.last);  // stage combine
      }
      state_t yn[14];
#pragma unroll
      for (int c = 0; c < 14; ++c) yn[c] = rk4_combine(LY(ln, c), dt_sixth, acc[c], k[c]);
      {  // normalize_quaternion (:227)
        const state_t n2 = ((yn[6] * yn[6] + yn[7] * yn[7]) + yn[8] * yn[8]) + yn[9] * yn[9];
#if ERPL_FAITHFUL
        const real nrm = m_sqrt(n2);
        if (nrm > (real)1e-12) { yn[6] /= nrm; yn[7] /= nrm; yn[8] /= nrm; yn[9] /= nrm; }
        else { yn[6] = 1; yn[7] = 0; yn[8] = 0; yn[9] = 0; }
#else
        const state_t r = m_rsq(n2);
        yn[6] *= r; yn[7] *= r; yn[8] *= r; yn[9] *= r;
        if (!(n2 > (state_t)1e-24)) { ERPL_RARE_BLOCK(); yn[6] = 1; yn[7] = 0; yn[8] = 0; yn[9] = 0; }  // |q| <= 1e-12 or NaN
#endif
      }
#pragma unroll
      for (int c = 0; c < 14; ++c) LY(ln, c) = yn[c];
#if ERPL_T_IN_LDS
      const double t_now = *tl + dt;
      *tl = t_now;
#else
      ln.t += dt;
      const double t_now = ln.t;
#endif
      ln.steps++;
      ++steps_done;
      ERPL_STAMP(ss.seg[6], ss.last);  // final combine + normalise
      const state_t alt = yn[2], vz = yn[5];
      // ---- everything below is straight-line selects; the single branch at the end is taken only
      // when a lane ends or turns non-finite ----
      // running argmax of altitude; np.argmax returns the first NaN (:488-490)
      alt_nan = m_isnan(alt);
      {
        const bool upd = !ln.nan_seen && (alt_nan || alt > ln.apogee);
        ln.apogee = upd ? alt : ln.apogee;
        ln.apogee_t = upd ? t_now : ln.apogee_t;
        ln.nan_seen = ln.nan_seen || alt_nan;
      }
      {
        const real sp2 = (real)((yn[3] * yn[3] + yn[4] * yn[4]) + vz * vz);
        ln.max_speed2 = (sp2 > ln.max_speed2) ? sp2 : ln.max_speed2;
#if ERPL_HANDOFF
        // (a NaN speed: the non-finite paths below.  The altitude test keeps the air density of the NEXT step - the
        // troposphere formula has no lower clamp, environment.py:28-33 - in the range the speed bound was derived for)
        extreme = (sp2 > (real)(ERPL_HANDOFF_SPEED * ERPL_HANDOFF_SPEED)) || (alt < (real)-1e5);
#endif
      }
      // termination tests on the post-step state (:233-264).  Only WHETHER the lane ends is decided
      // here; which of the reasons applies is resolved after the hot loop, from the same state.
      const bool ground = (alt <= (real)0.5) && (vz <= 0);
      const bool too_high = alt > (real)100000.0;
      const bool go_on = !(ground || too_high);
      latch_now = go_on && (alt > (real)1000.0) && (vz < 0) && !ln.apogee_detected;
      if (latch_now) {  // once per trajectory
        ERPL_RARE_BLOCK();
        ln.apogee_detected = true;
        ln.latch_t = t_now;
        ln.first_apogee = ln.apogee;
        ln.first_apogee_t = ln.apogee_t;
        ln.max_coast = (alt > (real)50000.0) ? (real)60.0 : ((alt > (real)25000.0) ? (real)120.0 : (real)300.0);
      }
      if (ln.apogee_detected && (alt > (real)25000.0)) {  // coasting above 25 km after the latch (:251-259)
        ERPL_RARE_BLOCK();
        coast_out = go_on && (t_now - ln.latch_t > (double)ln.max_coast);
      }
      const bool out_of_time = !(t_now < max_time);
      ended = out_of_time || coast_out || (latch_now && stop_at_apogee) || too_high || ground;
      nonfinite = !ended && (!TRAJ || traj_fast_forward) && alt_nan && m_isnan(vz);
    }
    ERPL_STAMP(ss.seg[7], ss.last);  // events
#if ERPL_HANDOFF
    } while (!TRAJ && __ballot(ended || nonfinite || extreme || (ln.mode == kPhysics && ln.steps >= ln.stop_steps)) == 0ull);
#else
    } while (!TRAJ && __ballot(ended || nonfinite || (ln.mode == kPhysics && ln.steps >= ln.stop_steps)) == 0ull);
#endif
    if (ln.mode == kPhysics) {
#if ERPL_T_IN_LDS
      ln.t = *tl;
#endif
      if (ended || nonfinite || TRAJ) {
      int end = -1;
      if (ended) {  // priority of the reference's tests (:233-264)
        const state_t alt = LY(ln, 2), vz = LY(ln, 5);
        end = ERPL_END_MAX_TIME;
        if (coast_out) end = ERPL_END_COAST;
        if (latch_now && stop_at_apogee) end = ERPL_END_APOGEE;
        if (alt > (real)100000.0) end = ERPL_END_ALTITUDE;
        if ((alt <= (real)0.5) && (vz <= 0)) end = ERPL_END_GROUND;
      }
      // ---- non-finite trajectories (SURVEY fact 9): the reference drags them to max_time ----
      if (nonfinite) {
        if (m_isnan(LY(ln, 0)) && m_isnan(LY(ln, 1))) {
          // all of position is NaN: nothing observable changes any more; the remaining loop is
          // `while t < max_time: t += dt`, tabulated on the host per rail-iteration count
          ColdArgs ca = cold_args();
          if (TRAJ) {   // (traj_fast_forward) this step's record, then one per stride with the time the loop would have
            traj_record<TRAJ>(ln, traj_len, false);
            while (ln.t < max_time) { ln.t += dt; ln.steps++; if (ln.t < max_time) traj_record<TRAJ>(ln, traj_len, false); }
          } else if (ln.nrail < ca->n_coast) {
            ln.t = ca->tables->coast_t[ln.nrail];
            ln.steps = ca->tables->coast_steps[ln.nrail];
          } else {
            while (ln.t < max_time) { ln.t += dt; ln.steps++; }
          }
          end = ERPL_END_MAX_TIME;
        } else {
          // z NaN, x or y still finite: with the motor off and a finite attitude the horizontal
          // acceleration is exactly 0 (q_dynamic is NaN -> no aero branch, thrust 0), so vx, vy stay
          // constant and x, y advance by the same RK4 increment every step: coast mode.
          const real pfc = (LY(ln, 13) > 0) ? (real)LY(ln, 13) : (real)0;
#if ERPL_T_IN_LDS
          const double burn_time = *bl;
#else
          const double burn_time = p.burn;
#endif
          const bool burning = (pfc > 0) && (ln.t <= burn_time);
          bool fin = true;
#pragma unroll
          for (int c = 6; c < 13; ++c) fin = fin && m_finite(LY(ln, c));
          if (!burning && fin) {
            const real vx = (real)LY(ln, 3), vy = (real)LY(ln, 4);
            ln.cx = ((vx + 2 * vx) + 2 * vx) + vx;
            ln.cy = ((vy + 2 * vy) + 2 * vy) + vy;
#if ERPL_STEP_COAST
            // fp64 builds: advance x, y step by step with the reference's rounding - unless the very first increment
            // already leaves both where they are (x, y infinite, NaN, or so large that the increment is below half an
            // ulp: the state of nearly every blown-up sample, e.g. [nan, -inf, nan]): the increments are constants, so
            // every later step is the same no-op and only t and the step count advance - the tabulated loop of the
            // all-NaN case above.  Exact, and it takes ~57 000 iterations per non-finite sample out of the kernel that
            // finishes the blow-ups (round 4: the hand-over sweep spent 7.5 ms per batch in them, profiles/r4_*).
            const state_t x0 = LY(ln, 0), y0 = LY(ln, 1);
            const state_t x1 = rk4_combine(x0, dt_sixth, ln.cx, (real)0), y1 = rk4_combine(y0, dt_sixth, ln.cy, (real)0);
            const bool still = ((x1 == x0) || (m_isnan(x1) && m_isnan(x0))) && ((y1 == y0) || (m_isnan(y1) && m_isnan(y0)));
            if (still) {
              ColdArgs cc = cold_args();
              if (TRAJ) {
                traj_record<TRAJ>(ln, traj_len, false);
                while (ln.t < max_time) { ln.t += dt; ln.steps++; if (ln.t < max_time) traj_record<TRAJ>(ln, traj_len, false); }
              } else if (ln.nrail < cc->n_coast) {
                ln.t = cc->tables->coast_t[ln.nrail];
                ln.steps = cc->tables->coast_steps[ln.nrail];
              } else {
                while (ln.t < max_time) { ln.t += dt; ln.steps++; }
              }
              end = ERPL_END_MAX_TIME;
            } else if (!TRAJ) {
              ln.mode = kCoast;   // (the capture build keeps stepping such a lane: the coast steps write no records)
            }
#else
            if (!TRAJ) {
            // fp32 path: the remaining steps add the same increment to x and y each time; do it in
            // closed form (closer to the fp64 reference than m sequential fp32 additions) and take
            // the final time / step count from the host table
            ColdArgs cc = cold_args();
            double tf = ln.t;
            int32_t total = ln.steps;
            if (ln.nrail < cc->n_coast) { tf = cc->tables->coast_t[ln.nrail]; total = cc->tables->coast_steps[ln.nrail]; }
            else { while (tf < max_time) { tf += dt; total++; } }
            const state_t m = (state_t)(total - ln.steps);
            LY(ln, 0) = LY(ln, 0) + m * (dt_sixth * (state_t)ln.cx);
            LY(ln, 1) = LY(ln, 1) + m * (dt_sixth * (state_t)ln.cy);
            ln.t = tf; ln.steps = total;
            end = ERPL_END_MAX_TIME;
            }
#endif
          }
        }
      }
      traj_record<TRAJ>(ln, traj_len, end >= 0);
      if (end >= 0) {
        if (TRAJ && ln.traj_slot >= 0) cold_args()->traj_len[ln.traj_slot] = traj_len;
        lane_finish(ln, end);
      }
      }  // rare path
    }
  }
  ColdArgs ca = cold_args();
#if ERPL_STAMPS
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) atomicAdd(&ca->counters[8 + i], ss.seg[i]);
  }
#endif
  if (lane == 0) atomicAdd(&ca->counters[2], wave_iters);
  // total physics steps: wave reduction then one atomic
  for (int off = 32; off > 0; off >>= 1) steps_done += __shfl_down(steps_done, off);
  if (lane == 0) atomicAdd(&ca->counters[1], steps_done);
}


#if ERPL_FAITHFUL
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
  const int64_t n = a.n, id = a.n_traj;
  LaneParams p;
  p.dry = (real)a.rocket[0 * n + id]; p.prop = (real)a.rocket[1 * n + id];
  p.thrust = (real)a.motor[0 * n + id]; p.Ae = (real)a.motor[1 * n + id];
  p.mdot = (real)a.motor[2 * n + id]; p.burn = a.motor[3 * n + id];
  lane_params_finish(S, p);
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
  real mass, cg, Ixx, Iyy;
  mass_props(S, p, y[13], mass, cg, Ixx, Iyy);
  o[3] = cg; o[4] = mass; o[5] = Ixx; o[6] = Iyy; o[7] = Iyy;
  real T, P;
  atmosphere(S, y[2], T, P);
  const real rho = P / (S.Rg * T);
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
  const real vb0 = (R00 * vr0 + R10 * vr1) + R20 * vr2;
  const real vb1 = (R01 * vr0 + R11 * vr1) + R21 * vr2;
  const real vb2 = (R02 * vr0 + R12 * vr1) + R22 * vr2;
  const real vn = m_sqrt((vr0 * vr0 + vr1 * vr1) + vr2 * vr2);
  const real mach = vn / m_sqrt((real)(1.4 * 287.053) * T);
  const bool a_dead = (m_abs(vb0) < (real)1e-6) && (m_abs(vb2) < (real)1e-6);
  const real vxz = m_sqrt(vb0 * vb0 + vb2 * vb2);
  const real alpha = a_dead ? (real)0 : m_atan2(vb2, vb0);
  const real beta = (vxz < (real)1e-6) ? (real)0 : m_atan2(vb1, vxz);
  MachCache mc;
  mach_cache_clear(mc);
  mach_lookup(C, mach, mc);
  real cd, cl, cy, cm, cyaw, cp_dyn;
  aero_coefficients(S, mach_rec_of(C, mc), mach, alpha, beta, cg, y[13] > 0, cd, cl, cy, cm, cyaw, cp_dyn);
  const real qdyn = ((real)0.5 * rho) * (vn * vn);
  real thrust = 0;  // motor.get_thrust(time[i], P) (motor.py:54-76 / :152-156)
  if (!(ts < 0.0 || ts > p.burn)) {
    if (C.motor_kind == ERPL_MOTOR_SOLID) thrust = solid_curve(C, (real)ts, p.thrust) + p.Ae * ((real)101325.0 - P);
    else thrust = p.thrust - p.Ae * P;
  }
  o[8] = thrust;
  o[9] = (qdyn * cd) * S.ref_area;
  o[10] = cd; o[11] = cl; o[12] = cm;
  o[13] = cp_dyn;
  o[14] = (cp_dyn - cg) / S.ref_diam;
  o[15] = alpha; o[16] = beta;
}
#endif  // ERPL_FAITHFUL

// ------------------------------------------------------------------------------------ debug kernel
// Known-answer evaluation on the device (erpl_mc_debug_eval; tests only): ONE function of the hot path
// per lane, through the very device functions the flight kernel inlines.  Lane j takes the per-sample
// parameters and wind table of sample j % n; in / out are [rows][m] doubles.
//   ERPL_DBG_ATMOSPHERE  in: altitude                        out: T, P, rho, g
//   ERPL_DBG_AERO        in: mach, alpha, beta, pf, power_on out: cd, cl, cy, cm, cyaw
//   ERPL_DBG_RHS         in: t, y[14], chute                 out: dy[14], chute
__global__ __launch_bounds__(256) void ERPL_CAT(erpl_debug_, ERPL_SUFFIX)(const ErplKArgs a, const ErplScalars<real> S,
                                                                         const int what, const int64_t m,
                                                                         const double* __restrict__ in,
                                                                         double* __restrict__ out) {
  __shared__ LdsTables L;
  __shared__ real alt_s[ERPL_MAX_WIND_KNOTS];
  stage_tables(L, alt_s, a.tables, a.alt_grid, a.k_wind);
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  Shared C;
  C.S = &S; C.L = &L; C.alt = alt_s; C.has_wind = a.k_wind > 0; C.motor_kind = a.motor_kind;
  const int64_t n = a.n, id = j % n;
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
#if ERPL_LDS_WIND
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
  } else {
    const double t = in[0 * m + j];
    real y[14], dy[14];
#pragma unroll
    for (int c = 0; c < 14; ++c) y[c] = (real)in[(1 + c) * m + j];
    bool chute = in[15 * m + j] > 0.0;
    StampSums ss;
#if ERPL_FAITHFUL
    rocket_dynamics(C, p, id, wc, mc, ac, chute, t, y, dy, ss);
#else
    rocket_dynamics(C, p, id, wc, mc, ac, chute, t, y, dy, ss, lr);
#endif
#pragma unroll
    for (int c = 0; c < 14; ++c) out[c * m + j] = (double)dy[c];
    out[14 * m + j] = chute ? 1.0 : 0.0;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------ launcher
int ERPL_LAUNCH_NAME(const ErplKArgs& a0, const void* scalars, int block, int max_blocks, int n_phases,
                     void* stream, void** ev, void* tail_stream, void* main_done) {
  hipStream_t st = (hipStream_t)stream;
  if (a0.n <= 0) return 0;
  ErplKArgs a = a0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  // One wave per workgroup for the rail kernel too: with several batches in flight every SIMD is full of flight
  // waves, and a 256-thread workgroup only starts once FOUR wave slots of one CU are free together, while the batch's
  // flight launch waits behind it (rocprofv3 timeline of bench.py: rail dispatches of 0.07 ms of work lasting 67-95 ms);
  // 64-thread workgroups slip into single slots as flight waves leave (bench shard: 27.08 -> 26.46 ms per pass over
  // five alternating runs, fp32 10.78 -> 10.61).
#ifndef ERPL_RAIL_BLOCK
#define ERPL_RAIL_BLOCK 64
#endif
  const int rail_block = ERPL_RAIL_BLOCK;
  const int64_t rail_grid = (a.n + rail_block - 1) / rail_block;
  if (ev) (void)hipEventRecord((hipEvent_t)ev[0], st);
  hipLaunchKernelGGL(ERPL_CAT(erpl_rail_, ERPL_SUFFIX), dim3((unsigned)rail_grid), dim3(rail_block), 0, st, a, S);
  if (ev) (void)hipEventRecord((hipEvent_t)ev[1], st);
#if ERPL_LANE_LDS
  if (block != kFlightBlock) {   // the per-lane LDS arrays are static [..][64]: this build always runs 64-thread workgroups
    if (max_blocks > 0) max_blocks = (int)(((int64_t)max_blocks * block + kFlightBlock - 1) / kFlightBlock);
    block = kFlightBlock;
  }
#endif
#if ERPL_DYN_ALT
  const size_t dyn_lds = (size_t)((a.k_wind > 0 ? a.k_wind : 1) * sizeof(real) + 15) & ~(size_t)15;
#else
  const size_t dyn_lds = 0;
#endif
  int64_t grid = (a.n + block - 1) / block;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  // One flight launch per step-chunk: the kernel boundary is the only synchronisation the
  // compaction needs.  Launches whose queue is already empty return at once.
  for (int ph = 0; ph < n_phases; ++ph) {
    a.phase = ph;
    a.adopt_lanes = (ph + 1 < n_phases && a0.n_traj == 0) ? a0.adopt_lanes : 0;   // the last launch flies everything out
    const dim3 g((unsigned)grid), b(block);
    const int spec = ((a.k_wind > 0) ? 1 : 0) | ((a.motor_kind == ERPL_MOTOR_SOLID) ? 2 : 0);
#define ERPL_LAUNCH_FLIGHT(TRAJ_, SPEC_, MINW_) \
    hipLaunchKernelGGL((ERPL_CAT(erpl_flight_, ERPL_SUFFIX)<TRAJ_, SPEC_, MINW_>), g, b, dyn_lds, st, a, S)
    if (a.n_traj > 0) ERPL_LAUNCH_FLIGHT(true, -1, ERPL_FLIGHT_MIN_WAVES);
#if ERPL_FAITHFUL || ERPL_FAST_F64
    else if (spec == 0) ERPL_LAUNCH_FLIGHT(false, 0, ERPL_FLIGHT_MIN_WAVES);
    else if (spec == 1) ERPL_LAUNCH_FLIGHT(false, 1, ERPL_FLIGHT_MIN_WAVES);
    else if (spec == 2) ERPL_LAUNCH_FLIGHT(false, 2, ERPL_FLIGHT_MIN_WAVES);
    else ERPL_LAUNCH_FLIGHT(false, 3, ERPL_FLIGHT_MIN_WAVES);
#else
    else if (a.waves_per_simd >= 3) {
      if (spec == 0) ERPL_LAUNCH_FLIGHT(false, 0, ERPL_DENSE_WAVES);
      else if (spec == 1) ERPL_LAUNCH_FLIGHT(false, 1, ERPL_DENSE_WAVES);
      else if (spec == 2) ERPL_LAUNCH_FLIGHT(false, 2, ERPL_DENSE_WAVES);
      else ERPL_LAUNCH_FLIGHT(false, 3, ERPL_DENSE_WAVES);
    } else {
      if (spec == 0) ERPL_LAUNCH_FLIGHT(false, 0, ERPL_FLIGHT_MIN_WAVES);
      else if (spec == 1) ERPL_LAUNCH_FLIGHT(false, 1, ERPL_FLIGHT_MIN_WAVES);
      else if (spec == 2) ERPL_LAUNCH_FLIGHT(false, 2, ERPL_FLIGHT_MIN_WAVES);
      else ERPL_LAUNCH_FLIGHT(false, 3, ERPL_FLIGHT_MIN_WAVES);
    }
#endif
#undef ERPL_LAUNCH_FLIGHT
    if (ph == 0 && tail_stream && n_phases > 1) {   // the sweeps follow the main launch on their own stream
      (void)hipEventRecord((hipEvent_t)main_done, st);
      st = (hipStream_t)tail_stream;
      (void)hipStreamWaitEvent(st, (hipEvent_t)main_done, 0);
    }
  }
#if ERPL_HANDOFF
  {  // the lanes this build handed over finish in the reference-order kernel, behind the last launch of the batch
    ErplKArgs g = a0;
    g.res_r[1] = a0.ext_r; g.res_d[1] = a0.ext_d; g.res_i[1] = a0.ext_i;
    g.qcnt = a0.ext_q; g.qhead = a0.ext_q + ERPL_EXT_Q;
    g.phase = 1; g.chunk_steps = 0; g.adopt_lanes = 0;
    const int rc = erpl_launch_f64_sweep(g, scalars, kWave, max_blocks, (void*)st);
    if (rc != 0) return rc;
  }
#endif
  if (ev) (void)hipEventRecord((hipEvent_t)ev[2], st);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

#if ERPL_FAITHFUL
// erpl_launch_f64_sweep (erpl_tables.h): the flight kernel alone (ERPL_SWEEP_MINW picks the instantiation), on the queue `a` maps
int erpl_launch_f64_sweep(const ErplKArgs& a, const void* scalars, int block, int max_blocks, void* stream) {
  if (a.n <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  int64_t grid = (a.n + block - 1) / block;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  const dim3 g((unsigned)grid), b(block);
  hipStream_t st = (hipStream_t)stream;
  const int spec = ((a.k_wind > 0) ? 1 : 0) | ((a.motor_kind == ERPL_MOTOR_SOLID) ? 2 : 0);
// Which instantiation flies the handed-over lanes: 1 = the gate's own (one wave per SIMD, all 512 registers, no scratch),
// 2 = a copy capped at 256 registers whose waves fit beside the throughput kernel's (612-772 bytes of scratch per lane,
// saved and restored around every exit of its RK4 loop).  Round 4 first shipped 2 on the idea that a 512-register wave would
// wait for an empty SIMD; measured side by side it does not cost a thing (22.41 / 23.30 ms per pass with 2, 22.81 / 22.68
// with 1) and the capped copy wrote 258 MB and fetched 226 MB per pass where this one writes 48 and fetches 103.
#ifndef ERPL_SWEEP_MINW
#define ERPL_SWEEP_MINW 1
#endif
#define ERPL_LAUNCH_SWEEP(TRAJ_, SPEC_) hipLaunchKernelGGL((erpl_flight_f64<TRAJ_, SPEC_, ERPL_SWEEP_MINW>), g, b, 0, st, a, S)
  if (a.n_traj > 0) ERPL_LAUNCH_SWEEP(true, -1);
  else if (spec == 0) ERPL_LAUNCH_SWEEP(false, 0);
  else if (spec == 1) ERPL_LAUNCH_SWEEP(false, 1);
  else if (spec == 2) ERPL_LAUNCH_SWEEP(false, 2);
  else ERPL_LAUNCH_SWEEP(false, 3);
#undef ERPL_LAUNCH_SWEEP
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int erpl_launch_extract_f64(const ErplKArgs& a, const void* scalars, double time_offset, void* stream) {
  if (a.traj_cap <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
  const int block = 256;
  const int64_t grid = (a.traj_cap + block - 1) / block;
  hipLaunchKernelGGL(erpl_extract_f64, dim3((unsigned)grid), dim3(block), 0, (hipStream_t)stream, a, S, time_offset);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
#endif

int ERPL_CAT(erpl_launch_debug_, ERPL_SUFFIX)(const ErplKArgs& a, const void* scalars, int what, int64_t m,
                                              const double* in, double* out, void* stream) {
  if (m <= 0) return 0;
  const ErplScalars<real> S = *(const ErplScalars<real>*)scalars;
#if ERPL_LDS_WIND
  const int block = kWave;   // per-lane LDS arrays of one wave
#else
  const int block = 256;
#endif
  const int64_t grid = (m + block - 1) / block;
  hipLaunchKernelGGL(ERPL_CAT(erpl_debug_, ERPL_SUFFIX), dim3((unsigned)grid), dim3(block), 0, (hipStream_t)stream, a, S,
                     what, m, in, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
