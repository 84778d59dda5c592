// erpl_k_lookup.h — what a lane looks things up in: the kernel arguments read at the point of use, the workgroup's LDS
// tables, the per-sample parameters, the cached wind / Mach / atmosphere intervals and (fp64 throughput build) the
// lane's handle on its LDS-resident data; with them the reference's models that more than one kernel evaluates.
namespace {

enum { kIdle = 0, kPhysics = 1, kCoast = 2 };                                  // lane modes
enum { kRecChute = 1, kRecNanSeen = 2, kRecApogee = 4, kRecFresh = 8 };       // record flag bits

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
#if ERPL_FAST_F64
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
};

// `alt` = the workgroup's copy of the wind altitude grid (static, or dynamic LDS of k_wind values)
__device__ __forceinline__ void stage_tables(LdsTables& L, real* alt, const ErplTables* __restrict__ T,
                                             const double* __restrict__ alt_grid, int k_wind) {
  const int tid = threadIdx.x, nt = blockDim.x;
#if ERPL_FAST_F64
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
#if ERPL_FAST_F64
// A record of a workgroup table as the lane keeps it: its BYTE offset in the table.  The table's own LDS address is a
// link-time constant that folds into the immediate offset of every read, so the lane's one register is the address
// register of all of them (an index costs a multiply and a shift per RHS evaluation).  Records are 16-byte aligned.
// They are read as 16-byte pairs: the alignment then belongs to the load itself (ds_read_b128 at base + immediate).
typedef real RealPair __attribute__((ext_vector_type(2)));
__device__ __forceinline__ const RealPair* lds_record(const real* table, int byte_off) {
  return (const RealPair*)((const char*)table + byte_off);
}
constexpr int kMachRecBytes = kMachRec * (int)sizeof(real), kAtmRecBytes = ERPL_ATM_REC * (int)sizeof(real);
static_assert(kMachRecBytes % 16 == 0 && kAtmRecBytes % 16 == 0, "table records are read 16 bytes at a time");
struct MachCache {
  int ro;   // kMachRecBytes x the number of union knots <= the Mach numbers of the interval; the record is read from the shared table
};
__device__ __forceinline__ void mach_cache_clear(MachCache& mc) { mc.ro = kMachEmpty * kMachRecBytes; }
__device__ __forceinline__ const real* mach_rec_of(const Shared& C, const MachCache& mc) { return (const real*)(lds_record(C.L->mach_rec, mc.ro) + 1); }
// the eight np.interp values of the lane's interval, for the RHS
__device__ __forceinline__ void mach_rec_load(const Shared& C, const MachCache& mc, real (&rec)[ERPL_MACH_REC]) {
  const RealPair* r = lds_record(C.L->mach_rec, mc.ro);
#pragma unroll
  for (int k = 0; k < ERPL_MACH_REC / 2; ++k) { const RealPair v = r[1 + k]; rec[2 * k] = v.x; rec[2 * k + 1] = v.y; }
}
__device__ __forceinline__ bool mach_inside(const Shared& C, const MachCache& mc, real mach) {
  const RealPair r = *lds_record(C.L->mach_rec, mc.ro);
  const real lo = r.x, hi = r.y;   // one 16-byte read, no short-circuit branch between the two
  return (mach >= lo) & (mach < hi);
}
__device__ __forceinline__ void mach_reload(const Shared& C, real mach, MachCache& mc) {
  const LdsTables& L = *C.L;
  const int n_union = cold_args()->n_union;
  // neighbour on the side the old interval was left, else count the knots (see the register variant below)
  int idx = mc.ro / kMachRecBytes + ((mach >= lds_record(L.mach_rec, mc.ro)->y) ? 1 : -1);
  idx = (idx < 0) ? 0 : ((idx > n_union) ? n_union : idx);
  if (!(mach >= L.mach_rec[idx * kMachRec] && mach < L.mach_rec[idx * kMachRec + 1])) {
    idx = 0;
    for (int j = 0; j < n_union; ++j) idx += (mach >= L.union_knots[j]) ? 1 : 0;
  }
  mc.ro = idx * kMachRecBytes;
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

// ------------------------------------------------------------------------------------ altitude-keyed data
#if ERPL_FAITHFUL
struct AtmCache { real lo, hi, alo, ahi; };  // unused by the faithful path (analytic piecewise atmosphere)
__device__ __forceinline__ void atm_cache_clear(AtmCache& ac) { ac.lo = 1; ac.hi = 0; ac.alo = 1; ac.ahi = 0; }
struct LaneRec { __device__ __forceinline__ void put_wind(const WindCache&) const {} };
#else
// Altitude-keyed data of this lane (fast path): the atmosphere layer record (environment.py:26-103 as
// one formula, see erpl_tables.h) and, through [lo, hi), the range of altitudes over which BOTH this
// record and the cached wind interval are valid - one range test per evaluation covers both tables;
// the reload (layer crossing or wind-knot crossing) is rare and reads LDS / HBM.
struct AtmCache {
  real lo, hi;     // altitudes over which BOTH the layer record and the cached wind interval hold
  real alo, ahi;   // altitudes of the layer alone: a wind-knot crossing inside it leaves the record as it is
#if ERPL_FAST_F64
  int ro;          // kAtmRecBytes x the layer index: the record is read from the workgroup's table where it is used
#else
  real r[10];  // aT bT Tlo Thi invTref eL href eH eM base
#endif
};
__device__ __forceinline__ void atm_cache_clear(AtmCache& ac) {
  ac.lo = 1; ac.hi = 0; ac.alo = 1; ac.ahi = 0;
#if ERPL_FAST_F64
  ac.ro = 0;
#endif
}

__device__ __forceinline__ void altitude_tables_reload(const Shared& C, int64_t id, real h, WindCache& wc, AtmCache& ac) {
  const ErplScalars<real>& S = *C.S;
  // (the cached layer bounds spare the fp32 build the record load; the fp64 build always takes it: erpl_k_config.h [5])
  if (!ERPL_FAST_F32 || !(h >= ac.alo && h < ac.ahi)) {   // layer crossing (or nothing cached yet, or NaN): four times per flight
    const int li = ((h > S.h_tropo) ? 1 : 0) + ((h > S.h_strat) ? 1 : 0) + ((h > (real)25000.0) ? 1 : 0) +
                   ((h > (real)32000.0) ? 1 : 0);  // NaN -> layer 0, whose formula propagates the NaN
#if ERPL_FAST_F64
    ac.ro = li * kAtmRecBytes;
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

// Handle of the lane's LDS-resident data for the RHS (fp64 throughput build): the wind interval is loaded right where the
// RHS consumes it (behind a compiler-level memory fence, so that the loads are not hoisted and held in registers
// through the evaluation); in the register builds the handle is empty and the calls vanish.  Layout: value k of
// lane l at lw[k * 64 + l] (conflict-free 8-byte reads).
enum { kLwLo = 0, kLwHi, kLwX0, kLwY0, kLwS = kLwY0 + 3, kLwSlots = kLwS + 3 };
struct LaneRec {
#if ERPL_FAST_F64
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
#endif

}  // namespace
