// erpl_k_flight.h — kernel 2: the flight integrator, with the lane's state (Lane) and the helpers that write a lane's
// trajectory records, results and resume-queue record.
namespace {

// ------------------------------------------------------------------------------------ kernel 2
struct Lane {
#if ERPL_FAST_F64
  real* yl;                  // the lane's state in LDS: values 2m, 2m+1 adjacent (one 16-byte read), pairs 64 lanes apart
#else
  real y[14];
#endif
  double t, t_rail;
  double apogee_t, first_apogee_t, latch_t;
  real apogee, first_apogee;
  real max_speed2, max_coast;
  real cx, cy;               // per-step x/y increments while coasting
  int64_t id;
  int64_t traj_slot;
  int32_t steps, nrail;
  int32_t mode;
  int32_t stop_steps;        // step count at which this launch parks the lane (chunking)
  bool chute, nan_seen, apogee_detected;
};

#if ERPL_FAST_F64
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
__device__ __forceinline__ void park_record(Lane& ln, int64_t traj_len, real* rr, double* rd, int32_t* ri, int64_t cap,
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
__device__ __forceinline__ real rk4_combine(real y, real dt_sixth, real acc, real k4) { return y + dt_sixth * (acc + k4); }

template <typename T> __device__ __forceinline__ bool m_finite(T x) { return (x - x) == (T)0; }

// SPEC >= 0 compiles the two launch-constant switches of the RHS in: bit 0 = a wind table is present,
// bit 1 = solid motor (thrust curve); SPEC < 0 reads them at run time (trajectory-capture build).
// MINW = waves per SIMD the register allocator must leave room for (ERPL_FLIGHT_MIN_WAVES, ERPL_DENSE_WAVES,
// ERPL_SWEEP_CAPPED_WAVES in erpl_k_config.h).
#if ERPL_FAST_F64
constexpr int kFlightBlock = kWave;   // per-lane LDS arrays of one wave: always 64-thread workgroups
constexpr bool kStepsAcrossLoop = true;
#else
constexpr int kFlightBlock = 256;
constexpr bool kStepsAcrossLoop = false;
#endif
template <bool TRAJ, int SPEC, int MINW>
__global__ __launch_bounds__(kFlightBlock, MINW) void ERPL_CAT(erpl_flight_, ERPL_SUFFIX)(const ErplKArgs a, const ErplScalars<real> S) {
  {  // a launch (or a workgroup) with nothing left in its queue leaves before touching anything
    // (records of this phase that waves of the previous launch already adopted are behind qhead; a
    // stale qhead only lets a workgroup too many start - block 0 never leaves while anything is queued)
    const unsigned long long n_in0 = (a.phase == 0) ? (unsigned long long)a.n : a.qcnt[a.phase];
    const unsigned long long taken0 = (a.phase == 0) ? 0ull : a.qhead[a.phase];
    if ((unsigned long long)blockIdx.x * blockDim.x >= n_in0 - (taken0 < n_in0 ? taken0 : n_in0)) return;
  }
  __shared__ LdsTables L;
#if ERPL_FAST_F64
  extern __shared__ double erpl_dyn_lds[];            // k_wind values (the launcher sizes it)
  real* const alt_s = (real*)erpl_dyn_lds;
#else
  __shared__ real alt_s[ERPL_MAX_WIND_KNOTS];
#endif
  stage_tables(L, alt_s, a.tables, a.alt_grid, a.k_wind);
  Shared C;
  C.S = &S;
  C.L = &L;
  C.alt = alt_s;
  C.has_wind = (SPEC < 0) ? (a.k_wind > 0) : ((SPEC & 1) != 0);
  C.motor_kind = (SPEC < 0) ? a.motor_kind : ((SPEC & 2) ? (int)ERPL_MOTOR_SOLID : (int)ERPL_MOTOR_LIQUID);
  const double dt = a.dt_flight, max_time = a.max_time;
  const real dt_sixth = S.dt_sixth, half_dt = S.half_dt, full_dt = S.dt_flight;
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
#if ERPL_FAST_F64   // the lane's state and wind interval in LDS (erpl_k_config.h [1])
  __shared__ __attribute__((aligned(16))) real lane_y[7][kWave][2];
  ln.yl = &lane_y[0][threadIdx.x][0];
  __shared__ real lane_wind[kLwSlots][kWave];
  lr.lw = &lane_wind[0][threadIdx.x];
#endif
#if ERPL_FAST_F32   // the lane's clock in LDS (erpl_k_config.h [4])
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

#if ERPL_FAST_F64
  bool extreme = false;
#endif
  for (;;) {
#if ERPL_FAST_F64
    // ---- hand-over: a lane that left the RK4 loop at an unphysical speed goes to the reference-order kernel
    // (erpl_k_config.h [2]); before the chunk / adoption parking below, which would send it round this kernel again ----
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
          park_record(ln, traj_len, (real*)ca->ext_r, ca->ext_d, ca->ext_i, ca->res_cap, base + (unsigned long long)rank);
        }
      }
      extreme = false;
    }
#endif
    // ---- compaction: lanes that used up their step chunk park their state densely in the next
    // phase's queue (one ballot-aggregated atomic per wave) and become idle ----
    {
      // lane adoption: with nothing left to refill from, a wave down to a few flying lanes costs almost
      // what a full one does (a half-empty wave issues 87-90 % of a full one's
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
          park_record(ln, traj_len, (real*)ca->res_r[(ph + 1) & 1], ca->res_d[(ph + 1) & 1], ca->res_i[(ph + 1) & 1], cap, e);
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
      const real* __restrict__ rr = (const real*)ca->res_r[src & 1];
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
#if ERPL_FAST_F32
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
            if (!(ln.t < max_time)) {  // while t < max_time never entered: the record above is the only one (:212-216)
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
#if ERPL_FAST_F32
    if (ln.mode == kPhysics) *tl = ln.t;
#endif
    // total physics steps, fp64 throughput build: a lane that integrates when the loop is entered does so until it is
    // left, one step per iteration, so its steps are the difference of ln.steps across the loop - not a 64-bit increment
    // (two vector instructions) in every step
    if (kStepsAcrossLoop && ln.mode == kPhysics) steps_done -= (unsigned long long)ln.steps;
    do {
    ++wave_iters;
    ended = false; nonfinite = false; alt_nan = false; latch_now = false; coast_out = false;
#if ERPL_FAST_F64
    extreme = false;
#endif
    if (!ERPL_FAST_F32 && ln.mode == kCoast) {   // the fp64 builds step their coasting lanes (the fp32 build: closed form, below)
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
#if ERPL_FAST_F32
        const double tb = *tl, burn = *bl;
#else
        const double tb = ln.t, burn = p.burn;
#endif
        const double th = tb + 0.5 * dt, tf = tb + dt;
        gates = ((tb <= burn) ? 1 : 0) | ((th <= burn) ? 2 : 0) | ((tf <= burn) ? 4 : 0);
        gates = (tb >= 0.0) ? gates : 0;   // no thrust before t = 0 (motor.py:54-57 / :152-153); th, tf >= tb: dt > 0 (host-checked)
        if (C.motor_kind == ERPL_MOTOR_SOLID) { gate_t[0] = (real)tb; gate_t[1] = (real)th; gate_t[2] = (real)tf; }
      }
#if ERPL_FAST_F32
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
        const real adv = (stage == 2) ? full_dt : half_dt;              // y + dt/2 k1, + dt/2 k2, + dt k3
        if (stage < 3) {
#pragma unroll
          for (int c = 0; c < 14; ++c) {
            acc[c] = (stage == 0) ? k[c] : acc[c] + wgt * k[c];
            ys[c] = LY(ln, c) + adv * k[c];
          }
        }
        ERPL_STAMP(ss.seg[5], ss.last);  // stage combine
      }
      real yn[14];
#pragma unroll
      for (int c = 0; c < 14; ++c) yn[c] = rk4_combine(LY(ln, c), dt_sixth, acc[c], k[c]);
      {  // normalize_quaternion (:227)
        const real n2 = ((yn[6] * yn[6] + yn[7] * yn[7]) + yn[8] * yn[8]) + yn[9] * yn[9];
#if ERPL_FAITHFUL
        const real nrm = m_sqrt(n2);
        if (nrm > (real)1e-12) { yn[6] /= nrm; yn[7] /= nrm; yn[8] /= nrm; yn[9] /= nrm; }
        else { yn[6] = 1; yn[7] = 0; yn[8] = 0; yn[9] = 0; }
#else
        const real r = m_rsq(n2);
        yn[6] *= r; yn[7] *= r; yn[8] *= r; yn[9] *= r;
        if (!(n2 > (real)1e-24)) { ERPL_RARE_BLOCK(); yn[6] = 1; yn[7] = 0; yn[8] = 0; yn[9] = 0; }  // |q| <= 1e-12 or NaN
#endif
      }
#pragma unroll
      for (int c = 0; c < 14; ++c) LY(ln, c) = yn[c];
#if ERPL_FAST_F32
      const double t_now = *tl + dt;
      *tl = t_now;
#else
      ln.t += dt;
      const double t_now = ln.t;
#endif
      ln.steps++;
      if (!kStepsAcrossLoop) ++steps_done;
      ERPL_STAMP(ss.seg[6], ss.last);  // final combine + normalise
      const real alt = yn[2], vz = yn[5];
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
#if ERPL_FAST_F64
        ln.max_speed2 = m_max(sp2, ln.max_speed2);   // (the running maximum is never NaN, and a NaN sp2 leaves it: the select below)
#else
        ln.max_speed2 = (sp2 > ln.max_speed2) ? sp2 : ln.max_speed2;
#endif
#if ERPL_FAST_F64
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
#if ERPL_FAST_F64
    } while (!TRAJ && __ballot(ended || nonfinite || extreme || (ln.mode == kPhysics && ln.steps >= ln.stop_steps)) == 0ull);
#else
    } while (!TRAJ && __ballot(ended || nonfinite || (ln.mode == kPhysics && ln.steps >= ln.stop_steps)) == 0ull);
#endif
    if (ln.mode == kPhysics) {
      if (kStepsAcrossLoop) steps_done += (unsigned long long)ln.steps;   // (before the fast-forward of a non-finite lane below moves ln.steps)
#if ERPL_FAST_F32
      ln.t = *tl;
#endif
      if (ended || nonfinite || TRAJ) {
      int end = -1;
      if (ended) {  // priority of the reference's tests (:233-264)
        const real alt = LY(ln, 2), vz = LY(ln, 5);
        end = ERPL_END_MAX_TIME;
        if (coast_out) end = ERPL_END_COAST;
        if (latch_now && stop_at_apogee) end = ERPL_END_APOGEE;
        if (alt > (real)100000.0) end = ERPL_END_ALTITUDE;
        if ((alt <= (real)0.5) && (vz <= 0)) end = ERPL_END_GROUND;
      }
      // ---- non-finite trajectories: the reference drags them to max_time ----
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
#if ERPL_FAST_F32
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
#if !ERPL_FAST_F32
            // fp64 builds: advance x, y step by step with the reference's rounding - unless the very first increment
            // already leaves both where they are (x, y infinite, NaN, or so large that the increment is below half an
            // ulp: the state of nearly every blown-up sample, e.g. [nan, -inf, nan]): the increments are constants, so
            // every later step is the same no-op and only t and the step count advance - the tabulated loop of the
            // all-NaN case above.  Exact, and it takes ~57 000 iterations per non-finite sample out of the kernel that
            // finishes the blow-ups (round 4: the hand-over sweep spent 7.5 ms per batch in them, profiles/r4_*).
            const real x0 = LY(ln, 0), y0 = LY(ln, 1);
            const real x1 = rk4_combine(x0, dt_sixth, ln.cx, (real)0), y1 = rk4_combine(y0, dt_sixth, ln.cy, (real)0);
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
            const real m = (real)(total - ln.steps);
            LY(ln, 0) = LY(ln, 0) + m * (dt_sixth * ln.cx);
            LY(ln, 1) = LY(ln, 1) + m * (dt_sixth * ln.cy);
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

}  // namespace
