// erpl_api.hip — host side of the C ABI declared in include/erpl_mc.h: the context, its batches and tickets
// (sampling: erpl_sampling.hip; the analysis entry points: erpl_stats_api.hip; shared: erpl_host.h).
// Derives the device tables from erpl_config with the reference's own expressions (glibc libm,
// the same pow/exp CPython uses), owns the per-GPU workspace and enqueues the two kernels.
// There is deliberately no CPU execution path in this library.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "erpl_host.h"
#include "erpl_debris.h"

// The one error buffer of the library (erpl_host.h): every unit writes it through erpl_fail.
static thread_local char g_err[512] = "";

int erpl_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

namespace {

bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}
bool increasing(const double* v, int n) {
  for (int i = 1; i < n; ++i) if (!(v[i] > v[i - 1])) return false;
  return true;
}

// np.interp interval record of table (xp, fp, n) for abscissae in [u, next union knot)
void interval_record(const double* xp, const double* fp, int n, bool below_all, double u,
                     double& x0, double& y0, double& s) {
  if (below_all || u < xp[0]) { x0 = xp[0]; y0 = fp[0]; s = 0.0; return; }
  if (u >= xp[n - 1]) { x0 = xp[n - 1]; y0 = fp[n - 1]; s = 0.0; return; }
  int j = 0;
  while (j + 1 < n && xp[j + 1] <= u) ++j;
  x0 = xp[j]; y0 = fp[j];
  s = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);  // numpy arr_interp slope
}

template <typename R>
void convert_scalars(const ErplScalars<double>& a, ErplScalars<R>& b) {
#define X(name) b.name = (R)a.name;
  ERPL_SCALARS(X)
#undef X
}

int build_tables(const erpl_config& c, ErplTables& T) {
  memset(&T, 0, sizeof(T));
  if (c.n_cd < 1 || c.n_cd > ERPL_MAX_MACH_KNOTS || c.n_cp < 1 || c.n_cp > ERPL_MAX_MACH_KNOTS)
    return erpl_fail(ERPL_ERR_INVALID, "Mach table sizes out of range (n_cd=%d n_cp=%d)", c.n_cd, c.n_cp);
  if (!finite_all(c.cd_mach, c.n_cd) || !finite_all(c.cd0, c.n_cd) || !finite_all(c.cda, c.n_cd) ||
      !finite_all(c.cp_mach, c.n_cp) || !finite_all(c.cp_shift, c.n_cp))
    return erpl_fail(ERPL_ERR_INVALID, "non-finite aerodynamic table entry");
  if (!increasing(c.cd_mach, c.n_cd) || !increasing(c.cp_mach, c.n_cp))
    return erpl_fail(ERPL_ERR_INVALID, "Mach knots must be strictly increasing");
  if (c.motor_kind != ERPL_MOTOR_LIQUID && c.motor_kind != ERPL_MOTOR_SOLID)
    return erpl_fail(ERPL_ERR_INVALID, "unknown motor_kind %d", c.motor_kind);
  if (c.motor_kind == ERPL_MOTOR_SOLID) {
    if (c.n_curve < 1 || c.n_curve > ERPL_MAX_CURVE_KNOTS)
      return erpl_fail(ERPL_ERR_INVALID, "thrust curve size out of range (%d)", c.n_curve);
    if (!finite_all(c.curve_time, c.n_curve) || !finite_all(c.curve_thrust, c.n_curve) ||
        !increasing(c.curve_time, c.n_curve))
      return erpl_fail(ERPL_ERR_INVALID, "thrust curve must be finite with increasing time");
  }
  if (!(c.dt_initial > 0) || !std::isfinite(c.dt_initial) || !std::isfinite(c.max_time))
    return erpl_fail(ERPL_ERR_INVALID, "dt_initial must be positive and finite");
  // the kernels count steps in int32 and advance time by `t += dt`: a horizon of more than 2^30 steps
  // overflows the counter, and long before that dt drops below ulp(t) and the loop stops advancing
  // (the reference would spin for ever there too) - refuse it instead of hanging the GPU
  if (c.max_time > 0 && c.max_time / ((0.005 < c.dt_initial) ? 0.005 : c.dt_initial) > 1073741824.0)
    return erpl_fail(ERPL_ERR_INVALID, "max_time / dt exceeds 2^30 steps");

  ErplScalars<double>& s = T.s64;
  s.dq2 = pow(c.diameter / 4, 2.0);                    // rocket.py:122
  s.cg_dry = c.center_of_mass_dry;
  s.prop_cg = c.center_of_mass_dry - 0.5;              // rocket.py:116
  s.third = 4.0 / 12;                                  // rocket.py:121-123
  s.Ixx_dry = c.Ixx_dry; s.Iyy_dry = c.Iyy_dry;
  s.ref_area = c.reference_area; s.ref_diam = c.reference_diameter; s.cp_location = c.cp_location;
  const double fin_area = 0.5 * (c.fin_root_chord + c.fin_tip_chord) * c.fin_span;  // rocket.py:176
  s.AR = (fin_area > 0) ? 2 * pow(c.fin_span, 2.0) / fin_area : 0.0;                // rocket.py:177
  s.two_pi_AR = 2 * M_PI * s.AR;                                                   // rocket.py:180
  s.cos_sweep = cos(c.fin_sweep_angle);
  s.cos_sweep_c = (1e-6 > s.cos_sweep) ? 1e-6 : s.cos_sweep;                        // rocket.py:179
  s.AR_over_cos = s.AR / s.cos_sweep_c;
  s.stall_angle = 15.0 * (M_PI / 180.0);                                           // rocket.py:167-168
  s.max_angle = 45.0 * (M_PI / 180.0);
  s.inv_stall_span = 1.0 / (s.max_angle - s.stall_angle);
  s.chute_area = c.parachute_area; s.chute_cd = c.parachute_cd;
  s.chute_alt = c.parachute_deployment_altitude; s.power_off = c.power_off_drag_factor;
  s.P0 = c.sea_level_pressure; s.T0 = c.sea_level_temperature; s.lapse = c.temperature_lapse_rate;
  s.Rg = c.gas_constant; s.g0 = c.gravity; s.h_tropo = c.troposphere_height;
  s.h_strat = c.stratosphere_height; s.T_strat = c.stratosphere_temp;
  s.tropo_exp = c.gravity / (c.gas_constant * c.temperature_lapse_rate);           // environment.py:33
  s.p11 = c.sea_level_pressure * pow(c.stratosphere_temp / c.sea_level_temperature, s.tropo_exp);
  s.p20 = s.p11 * exp(-c.gravity * (c.stratosphere_height - c.troposphere_height) /
                      (c.gas_constant * c.stratosphere_temp));                     // environment.py:56-62
  s.p25 = s.p20 * exp(-c.gravity * 5000.0 / (c.gas_constant * c.stratosphere_temp)); // :72-75
  s.grad_exp = c.gravity / (c.gas_constant * 0.0028);                              // :81
  s.dt_rail = c.dt_initial;
  s.dt_flight = (0.005 < c.dt_initial) ? 0.005 : c.dt_initial;                     // simulator.py:209
  s.half_dt = 0.5 * s.dt_flight;
  s.dt_sixth = s.dt_flight / 6.0;
  s.max_time = c.max_time; s.rail_length = c.rail_length;
  s.pitch_damping = c.pitch_damping; s.yaw_damping = c.yaw_damping;
  s.inv_T0 = 1.0 / s.T0; s.inv_Ts = 1.0 / s.T_strat; s.inv_Rg = 1.0 / s.Rg;
  s.k_iso = -s.g0 / (s.Rg * s.T_strat) * M_LOG2E;
  s.k_meso = s.g0 * M_LOG2E / s.Rg;
  s.two_pi_AR_cos = s.two_pi_AR * s.cos_sweep;
  s.area_diam = s.ref_area * s.ref_diam;
  s.AR_over_cos2 = s.AR_over_cos * s.AR_over_cos;
  s.q_of_PM2 = 0.5 * (1.4 * 287.053) / s.Rg;
  s.chute_k = 0.5 * s.chute_cd * s.chute_area;
  convert_scalars(T.s64, T.s32);
  T.dt_rail = s.dt_rail; T.dt_flight = s.dt_flight; T.max_time = s.max_time;
  T.motor_kind = c.motor_kind;
  T.n_curve = (c.motor_kind == ERPL_MOTOR_SOLID) ? c.n_curve : 0;
  for (int i = 0; i < T.n_curve; ++i) { T.curve_t[i] = c.curve_time[i]; T.curve_f[i] = c.curve_thrust[i]; }

  // union of the Cd and CP-shift Mach knots and the per-interval np.interp records
  std::vector<double> u(c.cd_mach, c.cd_mach + c.n_cd);
  u.insert(u.end(), c.cp_mach, c.cp_mach + c.n_cp);
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  T.n_union = (int)u.size();
  for (int i = 0; i < T.n_union; ++i) T.union_knots[i] = u[i];
  for (int i = 0; i <= T.n_union; ++i) {
    double* r = &T.mach_rec[i * ERPL_MACH_REC];
    const bool below = (i == 0);
    const double left = below ? u[0] : u[i - 1];
    double x0, y0, sl;
    interval_record(c.cd_mach, c.cd0, c.n_cd, below, left, x0, y0, sl);
    r[0] = x0; r[1] = y0; r[2] = sl;
    interval_record(c.cd_mach, c.cda, c.n_cd, below, left, x0, y0, sl);
    r[3] = y0; r[4] = sl;
    interval_record(c.cp_mach, c.cp_shift, c.n_cp, below, left, x0, y0, sl);
    r[5] = x0; r[6] = y0; r[7] = sl;
  }

  {  // atmosphere layer records for the fast path (see erpl_tables.h)
    const double inf = INFINITY;
    auto rec = [&](int k, double aT, double bT, double Tlo, double Thi, double invTref, double eL,
                   double href, double eH, double eM, double base) {
      double* r = &T.atm_rec[k * ERPL_ATM_REC];
      r[0] = aT; r[1] = bT; r[2] = Tlo; r[3] = Thi; r[4] = invTref; r[5] = eL;
      r[6] = href; r[7] = eH; r[8] = eM; r[9] = base; r[10] = 0; r[11] = 0;
    };
    rec(0, -s.lapse, s.T0, -inf, inf, s.inv_T0, s.tropo_exp, 0.0, 0.0, 0.0, s.P0);
    rec(1, 0.0, s.T_strat, -inf, inf, s.inv_Ts, 0.0, s.h_tropo, s.k_iso, 0.0, s.p11);
    rec(2, 0.001, s.T_strat - 0.001 * s.h_strat, -inf, 228.65, s.inv_Ts, 0.0, s.h_strat, s.k_iso, 0.0, s.p20);
    rec(3, 0.001, s.T_strat - 0.001 * s.h_strat, -inf, 228.65, s.inv_Ts, s.grad_exp, s.h_strat, 0.0, 0.0, s.p25);
    rec(4, -0.0028, 228.65 + 0.0028 * 32000.0, 180.0, inf, 1.0 / 228.65, 0.0, 32000.0, 0.0, -s.k_meso, 868.02);
  }

  // NaN fast-forward table (see erpl_tables.h): final t and step count of
  // `t = sum_r dt_rail; while t < max_time: t += dt_flight` per rail-iteration count r.
  T.n_coast = 0;
  const double est = (c.max_time > 0) ? c.max_time / s.dt_flight : 0;
  if (est < 2.0e6) {
    std::vector<double> t0(ERPL_COAST_TABLE);
    double t = 0.0;
    for (int r = 0; r < ERPL_COAST_TABLE; ++r) { t0[r] = t; t += s.dt_rail; }
    const int nthr = 8;   // (the values do not depend on the partition)
    const double dtf = s.dt_flight, tmax = c.max_time;
    run_threads(nthr, [&](int w) {
      for (int r = w; r < ERPL_COAST_TABLE; r += nthr) {
        double tt = t0[r];
        int32_t steps = 0;
        while (tt < tmax) { tt += dtf; ++steps; }
        T.coast_t[r] = tt;
        T.coast_steps[r] = steps;
      }
    });
    T.n_coast = ERPL_COAST_TABLE;
  }
  return ERPL_OK;
}

}  // namespace

// One workspace of the context: resume queues, queue cursors and counters of ONE batch in flight.
// Hardware queues the HIP runtime multiplexes this process's streams onto: GPU_MAX_HW_QUEUES, read by the
// runtime when it initialises (default 4).  Streams that share a queue run their kernels one after the
// other, so more batches in flight than queues is slower than three (measured at 131 072 samples, fp32:
// depth 4 / 4 queues 16.9 ms per batch, depth 4 / 8 queues 11.8 ms).  The library cannot ask the runtime;
// it trusts the environment variable the host set before the first HIP call (the Python package does).
static int hw_queues_env() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("GPU_MAX_HW_QUEUES");
    const int q = e ? atoi(e) : 0;
    v = q > 0 ? q : 4;
  }
  return v;
}


namespace {

// Whether the device has a second stream-priority pool, and the priority its streams are created at: asked when the lanes
// are about to take pool streams (erpl_sweep_stream of erpl_plan.h), once.  The greatest priority the device reports or the
// least made no difference that five rounds could tell: the greatest, so that the few waves of a
// tail are not the ones that wait.
bool other_priority_pool(erpl_ctx* c) {
  if (!c->pool_known) {
    int least = 0, greatest = 0;
    c->pool_exists = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest;
    c->pool_prio = greatest;
    c->pool_known = true;
  }
  return c->pool_exists;
}

void slot_free_workspace(ErplSlot& s) {
  for (int k = 0; k < 2; ++k) {
    (void)hipFree(s.res_r[k]); (void)hipFree(s.res_d[k]); (void)hipFree(s.res_i[k]);
    s.res_r[k] = nullptr; s.res_d[k] = nullptr; s.res_i[k] = nullptr;
  }
  (void)hipFree(s.ext_r); (void)hipFree(s.ext_d); (void)hipFree(s.ext_i);
  s.ext_r = nullptr; s.ext_d = nullptr; s.ext_i = nullptr; s.ext_cap = 0;
  s.cap = 0;
}

// The hand-over queue of the set (one more record buffer), for batches of the fp64 throughput build.
int slot_reserve_handoff(ErplSlot& s) {
  if (s.ext_cap >= s.cap) return ERPL_OK;
  if (s.used) HIP_TRY(hipEventSynchronize(s.done));
  (void)hipFree(s.ext_r); (void)hipFree(s.ext_d); (void)hipFree(s.ext_i);
  s.ext_r = nullptr; s.ext_d = nullptr; s.ext_i = nullptr; s.ext_cap = 0;
  const size_t rows = (size_t)s.cap;
  HIP_TRY(hipMalloc(&s.ext_r, rows * ERPL_RES_R * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&s.ext_d, rows * ERPL_RES_D * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&s.ext_i, rows * ERPL_RES_I * sizeof(int32_t)));
  s.ext_cap = s.cap;
  return ERPL_OK;
}

// Grows the slot's workspace to n samples.  The slot's previous batch may still be using the old one.
int slot_reserve(ErplSlot& s, int64_t n) {
  if (n <= s.cap) return ERPL_OK;
  if (s.used) HIP_TRY(hipEventSynchronize(s.done));
  slot_free_workspace(s);
  const size_t rows = (size_t)n;
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(hipMalloc(&s.res_r[k], rows * ERPL_RES_R * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&s.res_d[k], rows * ERPL_RES_D * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&s.res_i[k], rows * ERPL_RES_I * sizeof(int32_t)));
  }
  s.cap = n;
  return ERPL_OK;
}

int slot_init(ErplSlot& s) {
  if (s.d_queue) return ERPL_OK;
  HIP_TRY(hipMalloc((void**)&s.d_counters, 16 * sizeof(unsigned long long)));
  HIP_TRY(hipMalloc((void**)&s.d_queue, (2 * (ERPL_MAX_PHASES + 2) + 2 * ERPL_EXT_Q) * sizeof(unsigned long long)));
  HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&s.main_done, hipEventDisableTiming));
  HIP_TRY(hipHostMalloc((void**)&s.own_counters, 4 * sizeof(unsigned long long), hipHostMallocDefault));
  memset(s.own_counters, 0, 4 * sizeof(unsigned long long));
  s.h_counters = s.own_counters;
  return ERPL_OK;
}

void slot_destroy(ErplSlot& s) {
  slot_free_workspace(s);
  (void)hipFree(s.d_counters); (void)hipFree(s.d_queue);
  if (s.done) (void)hipEventDestroy(s.done);
  if (s.main_done) (void)hipEventDestroy(s.main_done);
  if (s.own_counters) (void)hipHostFree(s.own_counters);
  s = ErplSlot();
}

// The wind table of a batch as the kernels index it: 0..ERPL_MAX_WIND_KNOTS knots and, with knots, both buffers.
bool check_wind_args(const erpl_batch* b) {
  return b->k_wind >= 0 && b->k_wind <= ERPL_MAX_WIND_KNOTS && (b->k_wind == 0 || (b->alt_grid && b->wind));
}

int check_batch(const erpl_ctx* c, const erpl_batch* b, const erpl_out* o) {
  if (!c || !b || !o) return erpl_fail(ERPL_ERR_INVALID, "NULL argument");
  if (!c->has_cfg) return erpl_fail(ERPL_ERR_CONFIG, "erpl_mc_set_config has not been called");
  if (b->n < 0) return erpl_fail(ERPL_ERR_INVALID, "negative batch size");
  if (b->n == 0) return ERPL_OK;
  if (b->n > 2147483647LL) return erpl_fail(ERPL_ERR_INVALID, "at most 2^31 - 1 samples per batch");
  if (b->precision != ERPL_PREC_F64 && b->precision != ERPL_PREC_F32 && b->precision != ERPL_PREC_F64_FAST)
    return erpl_fail(ERPL_ERR_INVALID, "unknown precision %d", b->precision);
  if (b->k_wind < 0 || b->k_wind > ERPL_MAX_WIND_KNOTS)
    return erpl_fail(ERPL_ERR_INVALID, "k_wind %d out of range 0..%d", b->k_wind, ERPL_MAX_WIND_KNOTS);
  if (!b->ic || !b->rocket || !b->motor) return erpl_fail(ERPL_ERR_INVALID, "NULL input buffer");
  if (!check_wind_args(b)) return erpl_fail(ERPL_ERR_INVALID, "k_wind > 0 but no wind buffers");   // (the range is checked above)
  if (!o->summary || !o->status) return erpl_fail(ERPL_ERR_INVALID, "NULL output buffer");
  if (o->n_traj < 0 || (o->n_traj > 0 && (!o->traj_ids || !o->traj || !o->traj_len || o->traj_cap < 1 || o->traj_stride < 1)))
    return erpl_fail(ERPL_ERR_INVALID, "inconsistent trajectory-capture arguments");
  return ERPL_OK;
}

// Kernel arguments shared by every entry point that launches device code for a batch.
void fill_common_args(const erpl_ctx* c, const erpl_batch* b, ErplKArgs& a) {
  memset(&a, 0, sizeof(a));
  a.n = b->n; a.k_wind = b->k_wind; a.flags = b->flags;
  a.ic = b->ic; a.rocket = b->rocket; a.motor = b->motor; a.alt_grid = b->alt_grid; a.wind = b->wind;
  a.tables = c->d_tables;
  const ErplTables& T = c->h_tables;
  a.n_union = T.n_union; a.n_curve = T.n_curve; a.motor_kind = T.motor_kind; a.n_coast = T.n_coast;
  a.dt_rail = T.dt_rail; a.dt_flight = T.dt_flight; a.max_time = T.max_time;
}

// The step counter of the batches this context has FINISHED is copied to pinned memory behind every batch: what the
// choices that depend on trajectory length follow (kLongFlightSteps of erpl_plan.h).
void note_finished_batches(erpl_ctx* c) {
  for (int i = 0; i < 2 * ERPL_MAX_OVERLAP; ++i) {
    ErplSlot& q = c->slot[i];
    if (q.used && q.seq > c->seen_seq && q.last_n > 0 && hipEventQuery(q.done) == hipSuccess) {
      c->sched.seen_mean_steps = (double)q.h_counters[1] / (double)q.last_n;
      c->seen_seq = q.seq;
    }
  }
}

// What the policy of erpl_plan.h is told: the context's settings and history, the process and `n` samples of `precision`.
ErplPlanIn plan_inputs(const erpl_ctx* c, int precision, int64_t n) {
  ErplPlanIn in;
  static_cast<ErplSched&>(in) = c->sched;
  in.queues = hw_queues_env(); in.n_cu = c->n_cu;
  in.max_time = c->h_tables.max_time; in.dt_flight = c->h_tables.dt_flight;
  in.precision = precision; in.n = n;
  return in;
}

// The sweep stream of a lane for what is being submitted or reserved; latches the pool.
ErplSweepKind lane_sweep_kind(erpl_ctx* c, const ErplPlanIn& in) {
  return erpl_sweep_stream(in, c->pool_on, [c] { return other_priority_pool(c); });
}

// ... and a batch coming in through erpl_mc_run_batch or erpl_mc_submit_batch (before its sweep stream is known).
ErplPlanIn batch_inputs(erpl_ctx* c, const erpl_batch* b, const erpl_out* o, bool submit, int in_flight) {
  if (c->sched.chunk < 0) note_finished_batches(c);   // (automatic step chunks read seen_mean_steps)
  ErplPlanIn in = plan_inputs(c, b->precision, b->n);
  in.n_traj = o->n_traj; in.submit = submit; in.in_flight = in_flight;
  return in;
}

// Rail + flight kernels of one batch as `plan` says, through the lane's next set, on stream `st` (and the lane's sweep
// stream where the plan puts the launches behind the main one there); `ri` = the record of the batch's ticket in the
// ring, or -1 for erpl_mc_run_batch, which has none.
int enqueue_batch(erpl_ctx* c, int lane, const erpl_batch* b, const erpl_out* o, hipStream_t st, const ErplPlan& plan, int ri) {
  const int si = lane + ((plan.rotate_sets && (c->lane_uses[lane] & 1u)) ? ERPL_MAX_OVERLAP : 0);
  ErplSlot& s = c->slot[si];
  ERPL_TRY(slot_init(s));
  ERPL_TRY(slot_reserve(s, (b->n > c->reserve_n) ? b->n : c->reserve_n));
  // the slot's previous batch (possibly on another stream) must have drained its queues
  if (s.used) HIP_TRY(hipStreamWaitEvent(st, s.done, 0));
  // (queue cursors and counters are zeroed by the rail kernel itself)
  ErplKArgs a;
  fill_common_args(c, b, a);
  a.summary = o->summary; a.status = o->status;
  for (int k = 0; k < 2; ++k) { a.res_r[k] = s.res_r[k]; a.res_d[k] = s.res_d[k]; a.res_i[k] = s.res_i[k]; }
  a.res_cap = s.cap;
  a.qcnt = s.d_queue; a.qhead = s.d_queue + (ERPL_MAX_PHASES + 2);
  if (plan.handoff) {
    ERPL_TRY(slot_reserve_handoff(s));
    a.ext_r = s.ext_r; a.ext_d = s.ext_d; a.ext_i = s.ext_i;
  }
  a.ext_q = s.d_queue + 2 * (ERPL_MAX_PHASES + 2);
  a.ext_cnt = a.ext_q + 1;
  a.n_traj = o->n_traj; a.traj_stride = o->traj_stride; a.traj_cap = o->traj_cap;
  a.traj_ids = o->traj_ids; a.traj = o->traj; a.traj_len = o->traj_len;
  a.counters = s.d_counters;
  a.refill_threshold = c->refill;
  a.waves_per_simd = plan.waves_per_simd;
  a.chunk_steps = plan.chunk_steps;
  a.adopt_lanes = plan.adopt_lanes;
  a.adopt_spin = c->adopt_spin;
  const ErplTables& T = c->h_tables;
  const int max_blocks = c->max_blocks > 0 ? c->max_blocks : c->n_cu * 8 * (256 / c->block);
  void** ev = c->profiling ? (void**)&c->ev[3 * (c->profiled_runs % ERPL_PROFILE_RING)] : nullptr;
  hipStream_t tail = plan.tail_on_sweep ? c->lane_sweep[lane] : nullptr;
  int lrc;
  if (b->precision == ERPL_PREC_F64) lrc = erpl_launch_f64(a, &T.s64, c->block, max_blocks, plan.n_phases, st, ev, tail, s.main_done, plan.sweep_waves);
  else if (b->precision == ERPL_PREC_F64_FAST) lrc = erpl_launch_f64f(a, &T.s64, c->block, max_blocks, plan.n_phases, st, ev, tail, s.main_done, plan.sweep_waves);
  else lrc = erpl_launch_f32(a, &T.s32, c->block, max_blocks, plan.n_phases, st, ev, tail, s.main_done, plan.sweep_waves);
  if (c->profiling && lrc == 0) c->profiled_runs++;
  KERNEL_TRY(lrc);
  hipStream_t last = tail ? tail : st;
  s.h_counters = ri >= 0 ? &c->ring_counters[4 * ri] : s.own_counters;
  HIP_TRY(hipMemcpyAsync(s.h_counters, s.d_counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, last));
  HIP_TRY(hipEventRecord(s.done, last));
  if (ri >= 0) HIP_TRY(hipEventRecord(c->ring_done[ri], last));
  s.used = true;
  s.latest_is_run = ri < 0;
  s.last_n = b->n;
  s.last_plan = plan;
  s.seq = ++c->batches;
  c->last_slot = si;
  c->lane_uses[lane]++;
  return ERPL_OK;
}

// Waits for the most recent batch of the context and copies the first `words` of its device counters to h.
int fetch_last_counters(erpl_ctx* c, unsigned long long* h, int words) {
  HIP_TRY(hipSetDevice(c->device));
  const ErplSlot& ls = c->slot[c->last_slot];
  if (ls.used) HIP_TRY(hipEventSynchronize(ls.done));
  HIP_TRY(hipMemcpy(h, ls.d_counters, (size_t)words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return ERPL_OK;
}

int wait_all_host(erpl_ctx* c) {
  for (int i = 0; i < 2 * ERPL_MAX_OVERLAP; ++i)
    if (c->slot[i].used) HIP_TRY(hipEventSynchronize(c->slot[i].done));
  return ERPL_OK;
}

}  // namespace

extern "C" {

int erpl_mc_abi_version(void) { return ERPL_MC_ABI_VERSION; }
const char* erpl_mc_last_error(void) { return g_err; }

int erpl_mc_create(int device, erpl_ctx** out) {
  if (!out) return erpl_fail(ERPL_ERR_INVALID, "out is NULL");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return erpl_fail(ERPL_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= count) return erpl_fail(ERPL_ERR_INVALID, "device %d out of range (%d)", device, count);
  HIP_TRY(hipSetDevice(device));
  erpl_ctx* c = new erpl_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount;
  c->sched.depth = erpl_default_depth(hw_queues_env());
  hipError_t e = hipMalloc((void**)&c->d_tables, sizeof(ErplTables));
  for (int i = 0; i < 3 * ERPL_PROFILE_RING && e == hipSuccess; ++i) e = hipEventCreate(&c->ev[i]);
  if (e != hipSuccess) { (void)erpl_mc_destroy(c); return erpl_fail(ERPL_ERR_HIP, "hipMalloc/hipEventCreate: %s", hipGetErrorString(e)); }
  if (slot_init(c->slot[0]) != ERPL_OK) { (void)erpl_mc_destroy(c); return ERPL_ERR_HIP; }
  *out = c;
  return ERPL_OK;
}

int erpl_mc_destroy(erpl_ctx* c) {
  if (!c) return ERPL_OK;
  (void)hipSetDevice(c->device);
  (void)wait_all_host(c);
  (void)hipFree(c->d_tables);
  for (int i = 0; i < 2 * ERPL_MAX_OVERLAP; ++i) slot_destroy(c->slot[i]);
  for (int i = 0; i < ERPL_MAX_OVERLAP; ++i) {
    if (c->lane_stream[i]) (void)hipStreamDestroy(c->lane_stream[i]);
    if (c->lane_sweep[i]) (void)hipStreamDestroy(c->lane_sweep[i]);
    if (c->lane_in_ready[i]) (void)hipEventDestroy(c->lane_in_ready[i]);
  }
  for (int i = 0; i < 3 * ERPL_PROFILE_RING; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  for (int i = 0; i < ERPL_TICKET_RING; ++i) if (c->ring_done[i]) (void)hipEventDestroy(c->ring_done[i]);
  if (c->ring_counters) (void)hipHostFree(c->ring_counters);
  c->ana.release(); c->dist.release(); c->corr.release(); c->boot.release(); c->dens.release(); c->densw.release(); c->corridor.release(); c->sobol.release();
  c->dep.release(); c->cmp.release(); c->cmp_pop.release(); c->sur.release(); c->sur_model.release();
  (void)hipFree(c->legacy_buf);
  if (c->legacy_pin) (void)hipHostFree(c->legacy_pin);
  for (hipEvent_t e : c->legacy_ev) if (e) (void)hipEventDestroy(e);
  if (c->sur_pin) (void)hipHostFree(c->sur_pin);
  if (c->sur_ev) (void)hipEventDestroy(c->sur_ev);
  if (c->design_flag) (void)hipHostFree(c->design_flag);
  if (c->design_ev) (void)hipEventDestroy(c->design_ev);
  (void)hipFree(c->qmc_v);
  c->tally.release();
  c->subset.release();
  if (c->subset_pin) (void)hipHostFree(c->subset_pin);
  if (c->subset_ev) (void)hipEventDestroy(c->subset_ev);
  c->reweight.release();
  c->casualty.release();
  c->cdrv.release();
  c->depth.release();
  c->bands_w.release();
  if (c->reweight_pin) (void)hipHostFree(c->reweight_pin);
  delete c;
  return ERPL_OK;
}

int erpl_mc_set_config(erpl_ctx* c, const erpl_config* cfg) {
  if (!c || !cfg) return erpl_fail(ERPL_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());   // a batch still in flight on some stream reads the tables being replaced
  ErplTables& T = c->h_tables;
  c->has_cfg = false;
  ERPL_TRY(build_tables(*cfg, T));
  HIP_TRY(hipMemcpy(c->d_tables, &T, sizeof(T), hipMemcpyHostToDevice));
  c->has_cfg = true;
  return ERPL_OK;
}

int erpl_mc_reserve(erpl_ctx* c, int64_t n) {
  if (!c || n < 0) return erpl_fail(ERPL_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  if (n > c->reserve_n) c->reserve_n = n;
  // both workspaces of every lane in use now (erpl_mc_run_batch on lane 0 stays allocation-free, hence
  // graph-capturable, and no erpl_mc_submit_batch allocates in the middle of a run); lanes beyond the current depth
  // that have been used before grow too, fresh ones take the size on first use
  // (the second workspace of a lane is only ever used beside a sweep stream: without one the lane's next batch starts
  // behind the sweeps anyway, and it is not allocated - a workspace costs 448 bytes per sample)
  // (the same rule as erpl_mc_submit_batch, by the size asked for and for the build that can take a pool stream)
  const bool adopt = lane_sweep_kind(c, plan_inputs(c, kSweepPoolPrecision, n)) != ERPL_SWEEP_NONE;
  for (int i = 0; i < 2 * ERPL_MAX_OVERLAP; ++i) {
    if (i % ERPL_MAX_OVERLAP >= c->sched.depth && !c->slot[i].d_queue) continue;
    if (i >= ERPL_MAX_OVERLAP && !adopt && !c->slot[i].d_queue) continue;
    ERPL_TRY(slot_init(c->slot[i]));
    ERPL_TRY(slot_reserve(c->slot[i], c->reserve_n));
  }
  return ERPL_OK;
}

int erpl_mc_set_chunk(erpl_ctx* c, int chunk_steps) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  c->sched.chunk = chunk_steps < 0 ? -1 : chunk_steps;
  return ERPL_OK;
}

int erpl_mc_set_waves_per_simd(erpl_ctx* c, int waves) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (waves != 0 && waves != 2 && waves != 3) return erpl_fail(ERPL_ERR_INVALID, "waves per SIMD must be 0 (auto), 2 or 3");
  c->sched.waves = waves;
  return ERPL_OK;
}

int erpl_mc_set_adopt_spin(erpl_ctx* c, int polls) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "null context");
  c->adopt_spin = polls;
  return ERPL_OK;
}

int erpl_mc_set_adopt(erpl_ctx* c, int lanes) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "null context");
  if (lanes > 63) return erpl_fail(ERPL_ERR_INVALID, "adopt lanes must be at most 63");
  c->sched.adopt = lanes < 0 ? -1 : lanes;
  return ERPL_OK;
}

int erpl_mc_set_sweep_pool(erpl_ctx* c, int mode) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "null context");
  if (mode < -1 || mode > 1) return erpl_fail(ERPL_ERR_INVALID, "sweep pool mode must be -1 (by batch size), 0 (never) or 1 (always)");
  c->sched.sweep_pool = mode;
  if (mode == 0) c->pool_on = false;   // (streams and workspaces that exist stay; batches go back to the lane's one stream)
  return ERPL_OK;
}

int erpl_mc_set_launch(erpl_ctx* c, int block_threads, int max_blocks, int refill_threshold) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (block_threads != 64 && block_threads != 128 && block_threads != 256)
    return erpl_fail(ERPL_ERR_INVALID, "block_threads must be 64, 128 or 256");
  if (refill_threshold < 1 || refill_threshold > 64) return erpl_fail(ERPL_ERR_INVALID, "refill_threshold must be 1..64");
  c->block = block_threads;
  c->max_blocks = max_blocks < 0 ? 0 : max_blocks;
  c->refill = refill_threshold;
  return ERPL_OK;
}

int erpl_mc_run_batch(erpl_ctx* c, const erpl_batch* b, const erpl_out* o, void* stream) {
  int rc = check_batch(c, b, o);
  if (rc != ERPL_OK || b->n == 0) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return enqueue_batch(c, 0, b, o, (hipStream_t)stream, erpl_plan_batch(batch_inputs(c, b, o, false, 1)), -1);
}

int erpl_mc_get_overlap(erpl_ctx* c) { return c ? c->sched.depth : 0; }

int erpl_mc_set_overlap(erpl_ctx* c, int depth) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (depth < 1 || depth > ERPL_MAX_OVERLAP) return erpl_fail(ERPL_ERR_INVALID, "overlap depth must be 1..%d", ERPL_MAX_OVERLAP);
  HIP_TRY(hipSetDevice(c->device));
  ERPL_TRY(wait_all_host(c));
  c->sched.depth = depth;
  return ERPL_OK;
}

int erpl_mc_set_short_flight_overlap(erpl_ctx* c, int depth) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (depth < 0 || depth > ERPL_MAX_OVERLAP) return erpl_fail(ERPL_ERR_INVALID, "short-flight overlap must be 0..%d", ERPL_MAX_OVERLAP);
  c->short_depth = depth;
  return ERPL_OK;
}

int erpl_mc_submit_batch(erpl_ctx* c, const erpl_batch* b, const erpl_out* o, void* stream, int64_t* ticket) {
  ERPL_TRY(check_batch(c, b, o));
  if (ticket) *ticket = c->submitted;   // an empty batch is complete as soon as its predecessors are
  if (b->n == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  // Short flights (erpl_mc_set_short_flight_overlap) go round fewer lanes: fewer streams busy at a time
  int depth = c->sched.depth;
  if (c->short_depth > 0 && c->short_depth < depth) {
    note_finished_batches(c);
    if (c->sched.seen_mean_steps > 0.0 && c->sched.seen_mean_steps < kLongFlightSteps) depth = c->short_depth;
  }
  ErplPlanIn in = batch_inputs(c, b, o, true, depth);
  const int lane = (int)(c->submitted % depth);
  if (!c->lane_stream[lane]) HIP_TRY(hipStreamCreateWithFlags(&c->lane_stream[lane], hipStreamNonBlocking));
  // the lane's sweep stream, created with the first batch that gets one (a lane keeps the stream it has)
  const ErplSweepKind kind = in.sweep = lane_sweep_kind(c, in);
  if (kind != ERPL_SWEEP_NONE && !c->lane_sweep[lane]) {
    if (kind == ERPL_SWEEP_POOL) HIP_TRY(hipStreamCreateWithPriority(&c->lane_sweep[lane], hipStreamNonBlocking, c->pool_prio));
    else HIP_TRY(hipStreamCreateWithFlags(&c->lane_sweep[lane], hipStreamNonBlocking));
    c->lane_sweep_pool[lane] = kind == ERPL_SWEEP_POOL;
  }
  in.lane_stream_pool = c->lane_sweep_pool[lane];
  if (!c->lane_in_ready[lane]) HIP_TRY(hipEventCreateWithFlags(&c->lane_in_ready[lane], hipEventDisableTiming));
  // inputs written on the caller's stream so far are visible to the batch
  HIP_TRY(hipEventRecord(c->lane_in_ready[lane], (hipStream_t)stream));
  HIP_TRY(hipStreamWaitEvent(c->lane_stream[lane], c->lane_in_ready[lane], 0));
  // the ticket's own record: completion event + pinned counters (recycled ERPL_TICKET_RING tickets later)
  const int64_t t_new = c->submitted + 1;
  const int ri = (int)(t_new % ERPL_TICKET_RING);
  if (!c->ring_counters) {
    HIP_TRY(hipHostMalloc((void**)&c->ring_counters, ERPL_TICKET_RING * 4 * sizeof(unsigned long long), hipHostMallocDefault));
    memset(c->ring_counters, 0, ERPL_TICKET_RING * 4 * sizeof(unsigned long long));
  }
  if (!c->ring_done[ri]) HIP_TRY(hipEventCreateWithFlags(&c->ring_done[ri], hipEventDisableTiming));
  if (c->ring_ticket[ri] > 0) {   // the record of ticket t_new - ERPL_TICKET_RING leaves the ring: keep what nobody has been told yet
    HIP_TRY(hipEventSynchronize(c->ring_done[ri]));
    if (c->ring_counters[4 * ri + 3] != 0ull && c->ring_ticket[ri] > c->acked && c->recycled_incomplete == 0)
      c->recycled_incomplete = c->ring_ticket[ri];
  }
  for (int i = 0; i < 2 * ERPL_MAX_OVERLAP; ++i)   // (a set idle since that ticket must not read the record's next life)
    if (c->slot[i].h_counters == &c->ring_counters[4 * ri]) c->slot[i].h_counters = c->slot[i].own_counters;
  memset(&c->ring_counters[4 * ri], 0, 4 * sizeof(unsigned long long));
  c->ring_ticket[ri] = 0;
  ERPL_TRY(enqueue_batch(c, lane, b, o, c->lane_stream[lane], erpl_plan_batch(in), ri));
  c->ring_ticket[ri] = t_new;
  ++c->submitted;
  if (ticket) *ticket = c->submitted;
  return ERPL_OK;
}

namespace {
// the record of ticket t, or -1 once it has left the ring (then the batch has finished: recycling waited for it)
int ring_index(const erpl_ctx* c, int64_t t) {
  const int ri = (int)(t % ERPL_TICKET_RING);
  return (t > 0 && c->ring_ticket[ri] == t) ? ri : -1;
}
int report_incomplete(int64_t t, unsigned long long lost) {
  return erpl_fail(ERPL_ERR_INCOMPLETE, "lane hand-over timed out in batch %lld: %llu record(s) lost, their samples carry ERPL_ST_INCOMPLETE",
              (long long)t, lost);
}
// Blocking check of EVERY batch handed to the context so far; a failure is reported once: tickets up to the last one
// are acknowledged afterwards (erpl_mc_check_batch(T) keeps answering for T itself while T's record is in the ring).
int check_all(erpl_ctx* c) {
  ERPL_TRY(wait_all_host(c));
  ERPL_TRY(erpl_design_check_flag(c));
  int64_t bad = c->recycled_incomplete;
  unsigned long long lost = 0ull;
  for (int i = 0; i < ERPL_TICKET_RING; ++i) {
    const int64_t t = c->ring_ticket[i];
    if (t > c->acked && c->ring_counters[4 * i + 3] != 0ull && (bad == 0 || t < bad)) { bad = t; lost = c->ring_counters[4 * i + 3]; }
  }
  c->acked = c->submitted;
  c->recycled_incomplete = 0;
  if (bad > 0) return report_incomplete(bad, lost);
  for (int i = 0; i < 2 * ERPL_MAX_OVERLAP; ++i)   // erpl_mc_run_batch batches carry no ticket: the set's own copy
    if (c->slot[i].used && c->slot[i].latest_is_run && c->slot[i].own_counters[3] != 0ull)
      return report_incomplete(0, c->slot[i].own_counters[3]);
  return ERPL_OK;
}
}  // namespace

int erpl_mc_wait_batch(erpl_ctx* c, int64_t ticket, void* stream) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (ticket > c->submitted) return erpl_fail(ERPL_ERR_INVALID, "ticket %lld has not been handed out", (long long)ticket);
  HIP_TRY(hipSetDevice(c->device));
  if (ticket > 0) {
    // the ticket's own event (a ticket that has left the ring has finished: nothing to order behind)
    const int ri = ring_index(c, ticket);
    if (ri >= 0) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, c->ring_done[ri], 0));
  } else if (ticket < 0) {
    // every set's latest batch; a set is reused only behind its previous batch, so this covers all of them
    // (erpl_mc_run_batch's batches are ordered by the caller's own stream)
    for (int i = 0; i < 2 * ERPL_MAX_OVERLAP; ++i)
      if (c->slot[i].used && !c->slot[i].latest_is_run) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, c->slot[i].done, 0));
  }
  // the host does not block here, so only batches that have ALREADY finished can be reported (their counters sit in
  // pinned memory behind their event); erpl_mc_check_batch / erpl_mc_synchronize are the blocking checks
  if (c->recycled_incomplete > 0) return report_incomplete(c->recycled_incomplete, 0ull);
  for (int i = 0; i < ERPL_TICKET_RING; ++i) {
    const int64_t t = c->ring_ticket[i];
    if (t > c->acked && c->ring_counters[4 * i + 3] != 0ull && hipEventQuery(c->ring_done[i]) == hipSuccess)
      return report_incomplete(t, c->ring_counters[4 * i + 3]);
  }
  return ERPL_OK;
}

int erpl_mc_check_batch(erpl_ctx* c, int64_t ticket) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (ticket > c->submitted) return erpl_fail(ERPL_ERR_INVALID, "ticket %lld has not been handed out", (long long)ticket);
  HIP_TRY(hipSetDevice(c->device));
  if (ticket <= 0) return check_all(c);
  const int ri = ring_index(c, ticket);
  if (ri < 0) {   // older than the ring: finished long ago; what is left of it is the latch
    if (c->recycled_incomplete > 0) return report_incomplete(c->recycled_incomplete, 0ull);
    return ERPL_OK;
  }
  HIP_TRY(hipEventSynchronize(c->ring_done[ri]));   // this batch alone: later batches keep running
  if (c->ring_counters[4 * ri + 3] != 0ull) return report_incomplete(ticket, c->ring_counters[4 * ri + 3]);
  return ERPL_OK;
}

int erpl_mc_synchronize(erpl_ctx* c) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  HIP_TRY(hipSetDevice(c->device));
  return check_all(c);
}

int erpl_mc_set_profiling(erpl_ctx* c, int enable) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  c->profiling = enable != 0;
  c->profiled_runs = 0;
  return ERPL_OK;
}

int erpl_mc_kernel_ms_history(erpl_ctx* c, int max, float* rail_ms, float* flight_ms, int* n_out) {
  if (!c || !n_out || max < 0) return erpl_fail(ERPL_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  long long avail = c->profiled_runs < ERPL_PROFILE_RING ? c->profiled_runs : ERPL_PROFILE_RING;
  long long m = avail < max ? avail : max;
  for (long long k = 0; k < m; ++k) {
    const long long run = c->profiled_runs - m + k;
    hipEvent_t* e = &c->ev[3 * (run % ERPL_PROFILE_RING)];
    HIP_TRY(hipEventSynchronize(e[2]));
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
    HIP_TRY(hipEventElapsedTime(&b, e[1], e[2]));
    if (rail_ms) rail_ms[k] = a;
    if (flight_ms) flight_ms[k] = b;
  }
  *n_out = (int)m;
  return ERPL_OK;
}

int erpl_mc_last_kernel_ms(erpl_ctx* c, float* rail_ms, float* flight_ms) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (c->profiled_runs <= 0) return erpl_fail(ERPL_ERR_INVALID, "no profiled run_batch on this context");
  int n = 0;
  return erpl_mc_kernel_ms_history(c, 1, rail_ms, flight_ms, &n);
}

int erpl_mc_extract_histories(erpl_ctx* c, const erpl_batch* b, int64_t sample, const double* traj, int64_t m,
                              double time_offset, double* out, void* stream) {
  if (!c || !b || !traj || !out) return erpl_fail(ERPL_ERR_INVALID, "NULL argument");
  if (!c->has_cfg) return erpl_fail(ERPL_ERR_CONFIG, "erpl_mc_set_config has not been called");
  if (b->precision != ERPL_PREC_F64 && b->precision != ERPL_PREC_F64_FAST)
    return erpl_fail(ERPL_ERR_INVALID, "history extraction needs a batch with fp64 wind tables");
  if (sample < 0 || sample >= b->n || m < 0) return erpl_fail(ERPL_ERR_INVALID, "sample/m out of range");
  if (!check_wind_args(b)) return erpl_fail(ERPL_ERR_INVALID, "bad wind arguments");
  if (m == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  const ErplTables& T = c->h_tables;
  ErplKArgs a;
  fill_common_args(c, b, a);
  a.summary = out; a.traj = const_cast<double*>(traj); a.traj_cap = m; a.n_traj = sample;
  KERNEL_TRY(erpl_launch_extract_f64(a, &T.s64, time_offset, stream));
  return ERPL_OK;
}

int erpl_mc_flight_envelope(erpl_ctx* c, const erpl_batch* b, const erpl_out* o, double* envelope, void* stream) {
  if (!b) return erpl_fail(ERPL_ERR_INVALID, "NULL batch");
  if (!o) return erpl_fail(ERPL_ERR_INVALID, "NULL out");
  if (!envelope) return erpl_fail(ERPL_ERR_INVALID, "NULL envelope");
  if (b->precision != ERPL_PREC_F64 && b->precision != ERPL_PREC_F64_FAST)
    return erpl_fail(ERPL_ERR_INVALID, "precision = %d: the flight envelope needs a batch with fp64 wind tables", b->precision);
  if (b->n <= 0) return erpl_fail(ERPL_ERR_INVALID, "batch n = %lld: at least one sample", (long long)b->n);
  if (o->n_traj < 0 || o->n_traj > 2147483647LL)
    return erpl_fail(ERPL_ERR_INVALID, "n_traj = %lld out of range 0..2^31 - 1", (long long)o->n_traj);
  if (o->n_traj > 0) {
    if (o->traj_cap < 1) return erpl_fail(ERPL_ERR_INVALID, "traj_cap = %lld: at least one record per trajectory", (long long)o->traj_cap);
    if (!o->traj_ids) return erpl_fail(ERPL_ERR_INVALID, "NULL traj_ids");
    if (!o->traj) return erpl_fail(ERPL_ERR_INVALID, "NULL traj");
    if (!o->traj_len) return erpl_fail(ERPL_ERR_INVALID, "NULL traj_len");
    if (!b->rocket) return erpl_fail(ERPL_ERR_INVALID, "NULL rocket");
    if (!b->motor) return erpl_fail(ERPL_ERR_INVALID, "NULL motor");
    if (!check_wind_args(b)) return erpl_fail(ERPL_ERR_INVALID, "bad wind arguments (k_wind, alt_grid, wind)");
  }
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (!c->has_cfg) return erpl_fail(ERPL_ERR_CONFIG, "erpl_mc_set_config has not been called");
  if (o->n_traj == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  ErplKArgs a;
  fill_common_args(c, b, a);
  a.summary = envelope;
  a.n_traj = o->n_traj; a.traj_ids = o->traj_ids; a.traj_cap = o->traj_cap; a.traj = o->traj; a.traj_len = o->traj_len;
  KERNEL_TRY(erpl_launch_envelope_f64(a, &c->h_tables.s64, stream));
  return ERPL_OK;
}

int erpl_mc_impact_points_defaults(erpl_iip_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "NULL spec");
  memset(spec, 0, sizeof(*spec));
  spec->n_nodes = 64; spec->record_stride = 1; spec->max_steps = 20000;
  spec->dt = 0.05; spec->drag_scale = 1.0;
  return ERPL_OK;
}

int erpl_mc_impact_points(erpl_ctx* c, const erpl_batch* b, const erpl_out* o, const erpl_iip_spec* s, double* values,
                          int64_t ld, int64_t col0, double* summary, void* stream) {
  if (!b) return erpl_fail(ERPL_ERR_INVALID, "NULL batch");
  if (!o) return erpl_fail(ERPL_ERR_INVALID, "NULL out");
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "NULL spec");
  if (!values) return erpl_fail(ERPL_ERR_INVALID, "NULL values");
  if (s->n_nodes < 1 || s->n_nodes > ERPL_IIP_MAX_NODES)
    return erpl_fail(ERPL_ERR_INVALID, "n_nodes = %d out of range 1..%d", s->n_nodes, ERPL_IIP_MAX_NODES);
  if (s->record_stride < 1) return erpl_fail(ERPL_ERR_INVALID, "record_stride = %d: at least 1", s->record_stride);
  if (s->max_steps < 1 || s->max_steps > ERPL_IIP_MAX_STEPS)
    return erpl_fail(ERPL_ERR_INVALID, "max_steps = %d out of range 1..%d", s->max_steps, ERPL_IIP_MAX_STEPS);
  if (s->n_vertices != 0 && (s->n_vertices < 3 || s->n_vertices > ERPL_IIP_MAX_VERTICES))
    return erpl_fail(ERPL_ERR_INVALID, "n_vertices = %d: 0 or 3..%d", s->n_vertices, ERPL_IIP_MAX_VERTICES);
  if (!std::isfinite(s->dt) || !(s->dt > 0.0)) return erpl_fail(ERPL_ERR_INVALID, "dt = %g: finite and > 0", s->dt);
  if (!std::isfinite(s->ground)) return erpl_fail(ERPL_ERR_INVALID, "ground = %g: finite", s->ground);
  if (!std::isfinite(s->drag_scale) || !(s->drag_scale >= 0.0))
    return erpl_fail(ERPL_ERR_INVALID, "drag_scale = %g: finite and >= 0", s->drag_scale);
  if (!std::isfinite(s->origin_x)) return erpl_fail(ERPL_ERR_INVALID, "origin_x = %g: finite", s->origin_x);
  if (!std::isfinite(s->origin_y)) return erpl_fail(ERPL_ERR_INVALID, "origin_y = %g: finite", s->origin_y);
  for (int i = 0; i < s->n_vertices; ++i)
    if (!std::isfinite(s->keep_x[i]) || !std::isfinite(s->keep_y[i]))
      return erpl_fail(ERPL_ERR_INVALID, "keep-in vertex %d = (%g, %g): finite", i, s->keep_x[i], s->keep_y[i]);
  if (b->precision != ERPL_PREC_F64 && b->precision != ERPL_PREC_F64_FAST)
    return erpl_fail(ERPL_ERR_INVALID, "precision = %d: the impact points need a batch with fp64 wind tables", b->precision);
  if (b->n <= 0) return erpl_fail(ERPL_ERR_INVALID, "batch n = %lld: at least one sample", (long long)b->n);
  if (o->n_traj < 0 || o->n_traj > 2147483647LL)
    return erpl_fail(ERPL_ERR_INVALID, "n_traj = %lld out of range 0..2^31 - 1", (long long)o->n_traj);
  if (col0 < 0) return erpl_fail(ERPL_ERR_INVALID, "col0 = %lld: not negative", (long long)col0);
  if (ld - col0 < o->n_traj)   // (col0 >= 0: no overflow, and a negative ld is refused here too)
    return erpl_fail(ERPL_ERR_INVALID, "ld = %lld: the %lld columns from col0 = %lld on do not fit", (long long)ld,
                     (long long)o->n_traj, (long long)col0);
  if (o->n_traj > 0) {
    if (o->traj_cap < 1) return erpl_fail(ERPL_ERR_INVALID, "traj_cap = %lld: at least one record per trajectory", (long long)o->traj_cap);
    if (!o->traj_ids) return erpl_fail(ERPL_ERR_INVALID, "NULL traj_ids");
    if (!o->traj) return erpl_fail(ERPL_ERR_INVALID, "NULL traj");
    if (!o->traj_len) return erpl_fail(ERPL_ERR_INVALID, "NULL traj_len");
    if (!b->rocket) return erpl_fail(ERPL_ERR_INVALID, "NULL rocket");
    if (!b->motor) return erpl_fail(ERPL_ERR_INVALID, "NULL motor");
    if (!check_wind_args(b)) return erpl_fail(ERPL_ERR_INVALID, "bad wind arguments (k_wind, alt_grid, wind)");
  }
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (!c->has_cfg) return erpl_fail(ERPL_ERR_CONFIG, "erpl_mc_set_config has not been called");
  if (o->n_traj == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  ErplKArgs a;
  fill_common_args(c, b, a);
  a.n_traj = o->n_traj; a.traj_ids = o->traj_ids; a.traj_cap = o->traj_cap; a.traj = o->traj; a.traj_len = o->traj_len;
  ErplIipArgs q;
  q.n_nodes = s->n_nodes; q.record_stride = s->record_stride; q.max_steps = s->max_steps; q.reserved = 0;
  q.dt = s->dt; q.ground = s->ground; q.drag_scale = s->drag_scale; q.origin_x = s->origin_x; q.origin_y = s->origin_y;
  q.values = values; q.ld = ld; q.col0 = col0; q.summary = summary;
  ErplIipKeepIn keep;
  memset(&keep, 0, sizeof(keep));
  keep.n = s->n_vertices;
  for (int i = 0; i < s->n_vertices; ++i) { keep.x[i] = s->keep_x[i]; keep.y[i] = s->keep_y[i]; }
  KERNEL_TRY(erpl_launch_iip_f64(a, &c->h_tables.s64, q, keep, stream));
  return ERPL_OK;
}

int erpl_mc_debris_defaults(erpl_debris_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "NULL spec");
  memset(spec, 0, sizeof(*spec));
  spec->n_nodes = 16; spec->record_stride = 1; spec->max_steps = 20000; spec->n_fragments = 1;
  spec->dt = 0.05; spec->stiff_limit = 0.25;
  spec->beta[0] = (double)INFINITY;
  return ERPL_OK;
}

int erpl_mc_debris(erpl_ctx* c, const erpl_batch* b, const erpl_out* o, const erpl_debris_spec* s, double* values, int64_t ld,
                   int64_t col0, double* summary, void* stream) {
  if (!b) return erpl_fail(ERPL_ERR_INVALID, "NULL batch");
  if (!o) return erpl_fail(ERPL_ERR_INVALID, "NULL out");
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "NULL spec");
  if (!values) return erpl_fail(ERPL_ERR_INVALID, "NULL values");
  if (s->n_nodes < 1 || s->n_nodes > ERPL_IIP_MAX_NODES)
    return erpl_fail(ERPL_ERR_INVALID, "n_nodes = %d out of range 1..%d", s->n_nodes, ERPL_IIP_MAX_NODES);
  if (s->record_stride < 1) return erpl_fail(ERPL_ERR_INVALID, "record_stride = %d: at least 1", s->record_stride);
  if (s->max_steps < 1 || s->max_steps > ERPL_IIP_MAX_STEPS)
    return erpl_fail(ERPL_ERR_INVALID, "max_steps = %d out of range 1..%d", s->max_steps, ERPL_IIP_MAX_STEPS);
  if (s->n_vertices != 0 && (s->n_vertices < 3 || s->n_vertices > ERPL_IIP_MAX_VERTICES))
    return erpl_fail(ERPL_ERR_INVALID, "n_vertices = %d: 0 or 3..%d", s->n_vertices, ERPL_IIP_MAX_VERTICES);
  if (s->n_fragments < 1 || s->n_fragments > ERPL_DEBRIS_MAX_FRAGMENTS)
    return erpl_fail(ERPL_ERR_INVALID, "n_fragments = %d out of range 1..%d", s->n_fragments, ERPL_DEBRIS_MAX_FRAGMENTS);
  if ((int64_t)s->n_nodes * s->n_fragments > ERPL_CORRIDOR_MAX_NODES)
    return erpl_fail(ERPL_ERR_INVALID, "n_nodes * n_fragments = %lld: the product is at most %d rows per channel",
                     (long long)s->n_nodes * s->n_fragments, ERPL_CORRIDOR_MAX_NODES);
  if (!std::isfinite(s->dt) || !(s->dt > 0.0)) return erpl_fail(ERPL_ERR_INVALID, "dt = %g: finite and > 0", s->dt);
  if (!std::isfinite(s->ground)) return erpl_fail(ERPL_ERR_INVALID, "ground = %g: finite", s->ground);
  if (!std::isfinite(s->origin_x)) return erpl_fail(ERPL_ERR_INVALID, "origin_x = %g: finite", s->origin_x);
  if (!std::isfinite(s->origin_y)) return erpl_fail(ERPL_ERR_INVALID, "origin_y = %g: finite", s->origin_y);
  if (!(s->stiff_limit > 0.0 && s->stiff_limit <= 1.0))
    return erpl_fail(ERPL_ERR_INVALID, "stiff_limit = %g: in (0, 1]", s->stiff_limit);
  for (int f = 0; f < s->n_fragments; ++f) {
    if (!(s->beta[f] > 0.0)) return erpl_fail(ERPL_ERR_INVALID, "beta of fragment %d = %g: > 0 (+inf: no drag)", f, s->beta[f]);
    if (!std::isfinite(s->dv[f]) || !(s->dv[f] >= 0.0))
      return erpl_fail(ERPL_ERR_INVALID, "dv of fragment %d = %g: finite and >= 0", f, s->dv[f]);
  }
  for (int i = 0; i < s->n_vertices; ++i)
    if (!std::isfinite(s->keep_x[i]) || !std::isfinite(s->keep_y[i]))
      return erpl_fail(ERPL_ERR_INVALID, "keep-in vertex %d = (%g, %g): finite", i, s->keep_x[i], s->keep_y[i]);
  if (b->precision != ERPL_PREC_F64 && b->precision != ERPL_PREC_F64_FAST)
    return erpl_fail(ERPL_ERR_INVALID, "precision = %d: the debris footprint needs a batch with fp64 wind tables", b->precision);
  if (b->n <= 0) return erpl_fail(ERPL_ERR_INVALID, "batch n = %lld: at least one sample", (long long)b->n);
  if (o->n_traj < 0 || o->n_traj > 2147483647LL)
    return erpl_fail(ERPL_ERR_INVALID, "n_traj = %lld out of range 0..2^31 - 1", (long long)o->n_traj);
  if (col0 < 0) return erpl_fail(ERPL_ERR_INVALID, "col0 = %lld: not negative", (long long)col0);
  if (ld - col0 < o->n_traj)   // (col0 >= 0: no overflow, and a negative ld is refused here too)
    return erpl_fail(ERPL_ERR_INVALID, "ld = %lld: the %lld columns from col0 = %lld on do not fit", (long long)ld,
                     (long long)o->n_traj, (long long)col0);
  if (o->n_traj > 0) {
    if (o->traj_cap < 1) return erpl_fail(ERPL_ERR_INVALID, "traj_cap = %lld: at least one record per trajectory", (long long)o->traj_cap);
    if (!o->traj_ids) return erpl_fail(ERPL_ERR_INVALID, "NULL traj_ids");
    if (!o->traj) return erpl_fail(ERPL_ERR_INVALID, "NULL traj");
    if (!o->traj_len) return erpl_fail(ERPL_ERR_INVALID, "NULL traj_len");
    if (!b->rocket) return erpl_fail(ERPL_ERR_INVALID, "NULL rocket");
    if (!b->motor) return erpl_fail(ERPL_ERR_INVALID, "NULL motor");
    if (!check_wind_args(b)) return erpl_fail(ERPL_ERR_INVALID, "bad wind arguments (k_wind, alt_grid, wind)");
  }
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (!c->has_cfg) return erpl_fail(ERPL_ERR_CONFIG, "erpl_mc_set_config has not been called");
  if (o->n_traj == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  ErplKArgs a;
  fill_common_args(c, b, a);
  a.n_traj = o->n_traj; a.traj_ids = o->traj_ids; a.traj_cap = o->traj_cap; a.traj = o->traj; a.traj_len = o->traj_len;
  ErplDebrisArgs q;
  q.n_nodes = s->n_nodes; q.record_stride = s->record_stride; q.max_steps = s->max_steps; q.n_fragments = s->n_fragments;
  q.seed = s->seed;
  q.dt = s->dt; q.ground = s->ground; q.origin_x = s->origin_x; q.origin_y = s->origin_y; q.stiff_limit = s->stiff_limit;
  q.values = values; q.ld = ld; q.col0 = col0; q.summary = summary;
  ErplDebrisFragments fr;
  memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < s->n_fragments; ++f) { fr.beta[f] = s->beta[f]; fr.dv[f] = s->dv[f]; fr.order[f] = (uint8_t)f; }
  // the dispatch order: the lightest fragments (the longest falls) first
  std::stable_sort(fr.order, fr.order + s->n_fragments, [&](uint8_t x, uint8_t y) { return s->beta[x] < s->beta[y]; });
  ErplIipKeepIn keep;
  memset(&keep, 0, sizeof(keep));
  keep.n = s->n_vertices;
  for (int i = 0; i < s->n_vertices; ++i) { keep.x[i] = s->keep_x[i]; keep.y[i] = s->keep_y[i]; }
  KERNEL_TRY(erpl_launch_debris_f64(a, &c->h_tables.s64, q, fr, keep, stream));
  return ERPL_OK;
}

int erpl_mc_debris_directions_host(uint64_t seed, const int64_t* sample_ids, int64_t n, int32_t node, int32_t fragment,
                                   double* dir) {
  if (n < 0) return erpl_fail(ERPL_ERR_INVALID, "n = %lld: not negative", (long long)n);
  if (node < 0 || node >= ERPL_IIP_MAX_NODES) return erpl_fail(ERPL_ERR_INVALID, "node = %d out of range 0..%d", node, ERPL_IIP_MAX_NODES - 1);
  if (fragment < 0 || fragment >= ERPL_DEBRIS_MAX_FRAGMENTS)
    return erpl_fail(ERPL_ERR_INVALID, "fragment = %d out of range 0..%d", fragment, ERPL_DEBRIS_MAX_FRAGMENTS - 1);
  if (n > 0 && !sample_ids) return erpl_fail(ERPL_ERR_INVALID, "NULL sample_ids");
  if (n > 0 && !dir) return erpl_fail(ERPL_ERR_INVALID, "NULL dir");
  for (int64_t i = 0; i < n; ++i)
    if (sample_ids[i] < 0) return erpl_fail(ERPL_ERR_INVALID, "sample_ids[%lld] = %lld: not negative", (long long)i, (long long)sample_ids[i]);
  for (int64_t i = 0; i < n; ++i) {
    double d[3];
    erpl_debris_direction(seed, (uint64_t)sample_ids[i], (uint32_t)node, (uint32_t)fragment, d);
    for (int cc = 0; cc < 3; ++cc) dir[(int64_t)cc * n + i] = d[cc];
  }
  return ERPL_OK;
}

int erpl_mc_debug_eval(erpl_ctx* c, const erpl_batch* b, int what, int64_t m, const double* in, double* out, void* stream) {
  if (!c || !b || !in || !out) return erpl_fail(ERPL_ERR_INVALID, "NULL argument");
  if (!c->has_cfg) return erpl_fail(ERPL_ERR_CONFIG, "erpl_mc_set_config has not been called");
  if (what < ERPL_DBG_ATMOSPHERE || what > ERPL_DBG_MINMAX) return erpl_fail(ERPL_ERR_INVALID, "unknown function %d", what);
  if (what == ERPL_DBG_MINMAX && b->precision != ERPL_PREC_F64_FAST)   // (the other builds' kernels have no such branch)
    return erpl_fail(ERPL_ERR_INVALID, "ERPL_DBG_MINMAX: the fp64 throughput build only");
  if (b->n < 1 || m < 0 || !b->rocket || !b->motor) return erpl_fail(ERPL_ERR_INVALID, "need at least one sample with parameters");
  if (!check_wind_args(b)) return erpl_fail(ERPL_ERR_INVALID, "bad wind arguments");
  if (m == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  const ErplTables& T = c->h_tables;
  ErplKArgs a;
  fill_common_args(c, b, a);
  int rc;
  if (b->precision == ERPL_PREC_F64) rc = erpl_launch_debug_f64(a, &T.s64, what, m, in, out, stream);
  else if (b->precision == ERPL_PREC_F64_FAST) rc = erpl_launch_debug_f64f(a, &T.s64, what, m, in, out, stream);
  else if (b->precision == ERPL_PREC_F32) rc = erpl_launch_debug_f32(a, &T.s32, what, m, in, out, stream);
  else return erpl_fail(ERPL_ERR_INVALID, "unknown precision %d", b->precision);
  KERNEL_TRY(rc);
  return ERPL_OK;
}

int erpl_mc_debug_counters(erpl_ctx* c, double* out16) {
  if (!c || !out16) return erpl_fail(ERPL_ERR_INVALID, "NULL argument");
  unsigned long long h[16];
  ERPL_TRY(fetch_last_counters(c, h, 16));
  for (int i = 0; i < 16; ++i) out16[i] = (double)h[i];
  // host side, in the words no kernel counts in: what the library sized itself for and how it scheduled that batch
  const ErplSlot& ls = c->slot[c->last_slot];
  int streams = 0;
  for (int i = 0; i < ERPL_MAX_OVERLAP; ++i) streams += (c->lane_stream[i] != nullptr) + (c->lane_sweep[i] != nullptr);
  out16[4] = (double)hw_queues_env(); out16[5] = (double)streams;
  out16[6] = (double)ls.last_plan.adopt_lanes; out16[7] = (double)erpl_plan_word7(ls.last_plan);
  return ERPL_OK;
}

int erpl_mc_last_stats(erpl_ctx* c, double* total_steps, double* wave_iterations) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  unsigned long long h[4] = {0, 0, 0, 0};
  ERPL_TRY(fetch_last_counters(c, h, 4));
  if (total_steps) *total_steps = (double)h[1];
  if (wave_iterations) *wave_iterations = (double)h[2];
  if (h[3] != 0ull) return erpl_fail(ERPL_ERR_HIP, "lane hand-over timed out: the results of the last batch are incomplete");
  return ERPL_OK;
}

/* Device counters of ONE submitted batch (its record in the ticket ring): waits for that batch alone. */
int erpl_mc_ticket_stats(erpl_ctx* c, int64_t ticket, double* total_steps, double* wave_iterations) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  HIP_TRY(hipSetDevice(c->device));
  const int ri = ring_index(c, ticket);
  if (ri < 0) return erpl_fail(ERPL_ERR_INVALID, "ticket %lld is not (or no longer) among the last %d submitted batches",
                          (long long)ticket, (int)ERPL_TICKET_RING);
  HIP_TRY(hipEventSynchronize(c->ring_done[ri]));
  if (total_steps) *total_steps = (double)c->ring_counters[4 * ri + 1];
  if (wave_iterations) *wave_iterations = (double)c->ring_counters[4 * ri + 2];
  if (c->ring_counters[4 * ri + 3] != 0ull) return report_incomplete(ticket, c->ring_counters[4 * ri + 3]);
  return ERPL_OK;
}

}  // extern "C"
