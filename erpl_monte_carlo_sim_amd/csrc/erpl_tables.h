// erpl_tables.h — device-side constant tables shared by the host units (erpl_host.h) and the
// kernel translation units.  Everything here is derived on the HOST in fp64 from erpl_config
// with the reference's own expressions (so the values are bit-identical to what the Python
// reference recomputes on every call), then staged to LDS / scalar registers by the kernels.
#pragma once
#include <stdint.h>

#include "../../include/erpl_mc.h"

#define ERPL_MAX_UNION_KNOTS (2 * ERPL_MAX_MACH_KNOTS)
#define ERPL_MACH_REC 8         // x0a cd0_y0 cd0_s cda_y0 cda_s x0b cp_y0 cp_s
#define ERPL_ATM_LAYERS 5
#define ERPL_ATM_REC 12          // aT bT Tlo Thi invTref eL href eH eM base (2 pad)
#define ERPL_RES_R 20
#define ERPL_RES_D 5
#define ERPL_RES_I 6
#define ERPL_MAX_PHASES 2048
#define ERPL_EXT_Q 4            // words per cursor array of the hand-over queue (phases 0..3 of the sweep launch)
#define ERPL_COAST_TABLE 2048   // rail-iteration counts covered by the NaN fast-forward table

// Scalar constants, uniform over the batch.  X-macro so the fp64 master copy can be converted to
// the kernel's working precision field by field.
#define ERPL_SCALARS(X)                                                                        \
  X(dq2)            /* (diameter/4)**2                      rocket.py:122 */                    \
  X(cg_dry)         /* center_of_mass_dry                   rocket.py:31  */                    \
  X(prop_cg)        /* center_of_mass_dry - 0.5             rocket.py:116 */                    \
  X(third)          /* propellant_length**2 / 12 = 4/12     rocket.py:123 */                    \
  X(Ixx_dry) X(Iyy_dry)                                                                          \
  X(ref_area) X(ref_diam) X(cp_location)                                                         \
  X(AR)             /* 2 s^2 / fin_area                     rocket.py:177 */                    \
  X(two_pi_AR)      /* 2*pi*AR                              rocket.py:180 */                    \
  X(cos_sweep) X(cos_sweep_c) /* cos(sweep), max(cos(sweep),1e-6)  rocket.py:179-180 */         \
  X(AR_over_cos)    /* AR / cos_sweep_c (fast path only) */                                      \
  X(stall_angle) X(max_angle) X(inv_stall_span) /* radians(15), radians(45), 1/(max-stall) */    \
  X(chute_area) X(chute_cd) X(chute_alt) X(power_off)                                            \
  X(P0) X(T0) X(lapse) X(Rg) X(g0) X(h_tropo) X(h_strat) X(T_strat)                             \
  X(tropo_exp)      /* g/(R*lapse)                          environment.py:33 */                \
  X(p11) X(p20) X(p25) /* layer base pressures              environment.py:38-75 */             \
  X(grad_exp)       /* g/(R*0.0028)                         environment.py:81 */                \
  X(dt_rail) X(dt_flight) X(half_dt) X(dt_sixth) X(max_time) X(rail_length)                     \
  X(pitch_damping) X(yaw_damping)                                                                \
  /* host-folded constants used only by the fast (non-faithful) RHS */                           \
  X(inv_T0) X(inv_Ts) X(inv_Rg)                                                                  \
  X(k_iso)          /* -g/(R*T_strat) * log2(e)  : isothermal layers as exp2 */                  \
  X(k_meso)         /* g*log2(e)/R               : mesosphere scale-height term */               \
  X(two_pi_AR_cos)  /* 2*pi*AR*cos(sweep) */                                                     \
  X(area_diam)      /* reference_area * reference_diameter */                                    \
  X(chute_k)        /* 0.5 * parachute_cd * parachute_area */                                    \
  X(AR_over_cos2)   /* (AR / cos_sweep_c)^2 */                                                   \
  X(q_of_PM2)       /* 0.5 * (1.4 * 287.053) / R : q_dynamic = q_of_PM2 * P * Mach^2 */

template <typename R>
struct ErplScalars {
#define X(name) R name;
  ERPL_SCALARS(X)
#undef X
};

// Master tables in fp64 (device global memory); kernels convert while staging into LDS.
struct ErplTables {
  ErplScalars<double> s64;
  ErplScalars<float> s32;
  double dt_rail, dt_flight, max_time;  // fp64 copies for the time accumulation
  int32_t motor_kind, n_curve, n_union, n_coast;
  double curve_t[ERPL_MAX_CURVE_KNOTS], curve_f[ERPL_MAX_CURVE_KNOTS];
  double union_knots[ERPL_MAX_UNION_KNOTS];
  double mach_rec[(ERPL_MAX_UNION_KNOTS + 1) * ERPL_MACH_REC];
  // Atmosphere layers of environment.py:26-103 as one formula (fast path, LDS-staged):
  //   T = clamp(bT + aT*h, Tlo, Thi);  P = base * 2^( eL*log2(T*invTref) + (h-href)*(eH + eM/T) )
  double atm_rec[ERPL_ATM_LAYERS * ERPL_ATM_REC];
  // NaN fast-forward: a trajectory whose position is all-NaN can no longer trip any event
  // (every comparison is false), so it runs `while t < max_time: t += dt` to the end.  Its final
  // time and step count depend only on the number of rail iterations (t is an accumulated sum),
  // so the host tabulates them once per config.
  double coast_t[ERPL_COAST_TABLE];
  int32_t coast_steps[ERPL_COAST_TABLE];
};

// Arguments of both kernels (passed by value).
struct ErplKArgs {
  int64_t n;
  int32_t k_wind, flags;
  const double* ic;
  const double* rocket;
  const double* motor;
  const double* alt_grid;
  const void* wind;
  double* summary;
  int32_t* status;
  // Resume queue (ping-pong): lane records written by the rail kernel (phase 0) and by every flight
  // launch for the lanes that reached their step-chunk limit; the next launch pops them densely.
  void* res_r[2];              // [ERPL_RES_R][res_cap] working precision: y[14], apogee, first_apogee,
                               //   max_speed2, max_coast, cx, cy
  double* res_d[2];            // [ERPL_RES_D][res_cap]: t, t_rail, apogee_t, first_apogee_t, latch_t
  int32_t* res_i[2];           // [ERPL_RES_I][res_cap]: id, steps, nrail, mode|flags, traj_len, ready (the phase
                               //   that may pop the record, once it is published to running adopters)
  int64_t res_cap;
  unsigned long long* qcnt;    // [ERPL_MAX_PHASES + 2] records available to phase p (phase 0: n)
  unsigned long long* qhead;   // [ERPL_MAX_PHASES + 2] pop cursor of phase p
  // Hand-over queue (fp64 throughput build -> reference-order kernel, note [2] of erpl_k_config.h): records of
  // the lanes that left the RK4 loop at an unphysical speed, same layout and capacity as one resume-queue buffer.
  // The sweep launch of the reference-order kernel pops them as ITS phase 1: res_*[1] = ext_*, qcnt = ext_q
  // (ext_cnt = &ext_q[1]), qhead = ext_q + ERPL_EXT_Q.  NULL / unused in the other builds.
  void* ext_r;
  double* ext_d;
  int32_t* ext_i;
  unsigned long long* ext_q;   // [2 * ERPL_EXT_Q] behind qhead in the same allocation (zeroed by the rail kernel)
  unsigned long long* ext_cnt;
  int32_t phase;               // index of this flight launch
  int32_t chunk_steps;         // RK4 steps a lane may take per launch (<= 0: unlimited, one launch)
  int32_t waves_per_simd;      // fp32 flight-kernel build to launch: 2 (256 VGPRs) or 3 (168 VGPRs, spills)
  int32_t adopt_spin;          // polls an adopting lane waits for a claimed record's ready word (< 0: none - test knob)
  int32_t adopt_lanes;         // > 0: a wave left with at most this many flying lanes once the queue is empty
                               //   parks them in the next phase's queue, where waves that still fly more pick
                               //   them up into their idle lanes (the launcher clears it for the last phase)
  // trajectory capture
  int64_t n_traj, traj_stride, traj_cap;
  const int64_t* traj_ids;
  double* traj;
  int64_t* traj_len;
  const ErplTables* tables;
  unsigned long long* counters;  // [0] queue head, [1] total steps, [2] wave iterations
  int32_t refill_threshold;
  int32_t n_union, n_curve, motor_kind, n_coast;   // uniform table sizes (also in *tables)
  double dt_rail, dt_flight, max_time;             // fp64 time constants
};

// launchers implemented in erpl_k64.hip / erpl_k32.hip
extern "C++" {
// ev: NULL or three hipEvent_t recorded before the rail kernel, between the kernels and after the
// flight kernel, on `stream`.
// scalars: host pointer to ErplScalars<double> / ErplScalars<float>, passed to the kernels BY VALUE
// (kernel-argument segment -> scalar registers; a pointer into global memory would be re-read
// through the vector memory path on every use because the kernels also store to global memory).
// n_phases flight launches follow the rail launch (1 when a.chunk_steps <= 0).
// tail_stream (or NULL): the launches behind the first go to that stream, after main_done (a hipEvent_t recorded on
// `stream` behind the first launch).
// sweep_waves: erpl_launch_f64f passes it on to erpl_launch_f64_sweep; the other two ignore it.
int erpl_launch_f64(const ErplKArgs& a, const void* scalars, int block, int max_blocks, int n_phases, void* stream, void** ev,
                    void* tail_stream, void* main_done, int sweep_waves);
int erpl_launch_f32(const ErplKArgs& a, const void* scalars, int block, int max_blocks, int n_phases, void* stream, void** ev,
                    void* tail_stream, void* main_done, int sweep_waves);
int erpl_launch_f64f(const ErplKArgs& a, const void* scalars, int block, int max_blocks, int n_phases, void* stream, void** ev,
                    void* tail_stream, void* main_done, int sweep_waves);
// The sweep of the fp64 throughput build's hand-over queue by the reference-order flight kernel (no rail launch): `a` is
// the batch's argument block with the hand-over queue mapped as phase 1 (see ErplKArgs::ext_r).  waves = 1 runs the gate's
// own instantiation (one wave per SIMD, all 512 registers, no scratch): sweeps on a stream of their own,
// erpl_mc_run_batch, trajectory capture.  waves = 2 runs the copy capped at 256 registers, whose waves start beside the
// throughput kernel's: sweeps on the stream that carries the lane's next batch (note [3] of erpl_k_config.h).
int erpl_launch_f64_sweep(const ErplKArgs& a, const void* scalars, int block, int max_blocks, void* stream, int waves);
// known-answer evaluation of one device function per lane (erpl_mc_debug_eval); in / out are [rows][m]
int erpl_launch_debug_f64(const ErplKArgs& a, const void* scalars, int what, int64_t m, const double* in, double* out, void* stream);
int erpl_launch_debug_f32(const ErplKArgs& a, const void* scalars, int what, int64_t m, const double* in, double* out, void* stream);
int erpl_launch_debug_f64f(const ErplKArgs& a, const void* scalars, int what, int64_t m, const double* in, double* out, void* stream);
// extraction of the per-step diagnostic histories (fp64 only): a.traj = records, a.traj_cap = m,
// a.n_traj = sample index, a.summary = out [m][ERPL_DIAG_DIM]
int erpl_launch_extract_f64(const ErplKArgs& a, const void* scalars, double time_offset, void* stream);
// the flight envelope of every captured trajectory (fp64 only): a.n_traj / traj_ids / traj_cap / traj / traj_len as
// erpl_out has them, a.summary = envelope [ERPL_ENV_DIM][n_traj]; one workgroup per trajectory (n_traj < 2^31)
int erpl_launch_envelope_f64(const ErplKArgs& a, const void* scalars, void* stream);
}

// What the kernels of erpl_mc_impact_points take besides ErplKArgs (by value): the scalar fields of erpl_iip_spec and
// the caller's buffers; the keep-in vertices go to the summary kernel alone.
struct ErplIipArgs {
  int32_t n_nodes, record_stride, max_steps, reserved;
  double dt, ground, drag_scale, origin_x, origin_y;
  double* values;    // [ERPL_IIP_CH_COUNT][n_nodes][ld]
  int64_t ld, col0;
  double* summary;   // [ERPL_IIP_DIM][n_traj] or NULL
};
struct ErplIipKeepIn {
  int32_t n, reserved;
  double x[ERPL_IIP_MAX_VERTICES], y[ERPL_IIP_MAX_VERTICES];
};
extern "C++" {
// the instantaneous impact points of every captured trajectory (fp64 only): a.n_traj / traj_ids / traj_cap / traj / traj_len
// as erpl_out has them (n_traj < 2^31, q.n_nodes <= ERPL_IIP_MAX_NODES); the prefix kernel, the fall kernel, then
// (q.summary != NULL) the summary kernel, one behind the other on the same stream
int erpl_launch_iip_f64(const ErplKArgs& a, const void* scalars, const ErplIipArgs& q, const ErplIipKeepIn& keep, void* stream);
}

// What the kernels of erpl_mc_debris take besides ErplKArgs (by value): the scalar fields of erpl_debris_spec and the
// caller's buffers; the fragments go to the fall kernel alone, the keep-in vertices (ErplIipKeepIn) to the summary kernel.
struct ErplDebrisArgs {
  int32_t n_nodes, record_stride, max_steps, n_fragments;
  uint64_t seed;
  double dt, ground, origin_x, origin_y, stiff_limit;
  double* values;    // [ERPL_IIP_CH_COUNT][n_nodes * n_fragments][ld]
  int64_t ld, col0;
  double* summary;   // [ERPL_DEBRIS_DIM][n_traj] or NULL
};
struct ErplDebrisFragments {
  double beta[ERPL_DEBRIS_MAX_FRAGMENTS], dv[ERPL_DEBRIS_MAX_FRAGMENTS];
  uint8_t order[ERPL_DEBRIS_MAX_FRAGMENTS];   // the fragment dispatched r-th: ascending beta, ties by index
};
extern "C++" {
// the debris footprint of every captured trajectory (fp64 only): a.* as for erpl_launch_iip_f64; the prefix kernel, the fall
// kernel, then (q.summary != NULL) the summary kernel, one behind the other on the same stream
int erpl_launch_debris_f64(const ErplKArgs& a, const void* scalars, const ErplDebrisArgs& q, const ErplDebrisFragments& fr,
                           const ErplIipKeepIn& keep, void* stream);
}

// ---- erpl_mc_analyze: outlier filter + exact statistics on the summary (erpl_analysis.hip) ----
#define ERPL_ANA_BLOCK 256        // threads per workgroup of the streaming passes
#define ERPL_ANA_MAX_BLOCKS 1024  // their grid: min(this, ceil(n / ERPL_ANA_BLOCK)) - a function of n alone, so the
                                  //   reduction has the same shape on every device and in every call (bitwise repeatable)
#define ERPL_ANA_TARGETS (2 * ERPL_ANALYSIS_MAX_Q)   // order statistics selected per row: lo and hi of every quantile
#define ERPL_ANA_BINS 256         // one 8-bit digit per selection pass, most significant first
#define ERPL_ANA_COUNTERS 16      // [0..5] reason bits, [6..10] end codes, [11] ERPL_ST_NAN, [12] ERPL_ST_INCOMPLETE, [13] valid

// What the device hands back (copied to a pinned block, finished on the host).
struct ErplAnaRow {
  unsigned long long count;                   // valid samples finite in this row
  double sum, mean, m2, vmin, vmax;           // m2 = sum((x - mean)^2), second pass
  unsigned long long key[ERPL_ANA_TARGETS];   // order-preserving keys of the selected order statistics
};
struct ErplAnaResult {
  unsigned long long counter[ERPL_ANA_COUNTERS];
  ErplAnaRow row[ERPL_ANALYSIS_MAX_ROWS];
};
// Selection state of one row with NT targets (the passes: erpl_stat_device.h): what is fixed of every target's key so far,
// its rank among the keys that share that prefix, and the first target with the same prefix (targets that share a prefix
// share one histogram).
extern "C++" {
template <int NT>
struct ErplSelect {
  unsigned long long prefix[NT], rank[NT];
  int32_t leader[NT];
};
}
typedef ErplSelect<ERPL_ANA_TARGETS> ErplAnaSelect;
// The fixed part of the workspace (the per-sample reason bytes are a second allocation that grows with n).
struct ErplAnaWork {
  ErplAnaResult res;
  unsigned long long cpart[ERPL_ANA_MAX_BLOCKS][ERPL_ANA_COUNTERS];    // classify: counters per workgroup
  double psum[ERPL_ANALYSIS_MAX_ROWS][ERPL_ANA_MAX_BLOCKS];            // moments: partials per row and workgroup
  double pmin[ERPL_ANALYSIS_MAX_ROWS][ERPL_ANA_MAX_BLOCKS];
  double pmax[ERPL_ANALYSIS_MAX_ROWS][ERPL_ANA_MAX_BLOCKS];
  unsigned long long pcnt[ERPL_ANALYSIS_MAX_ROWS][ERPL_ANA_MAX_BLOCKS];
  ErplAnaSelect sel[ERPL_ANALYSIS_MAX_ROWS];
  unsigned long long hist[ERPL_ANALYSIS_MAX_ROWS][ERPL_ANA_TARGETS][ERPL_ANA_BINS];   // 64-bit digit histograms
};
struct ErplAnaArgs {
  const double* summary;   // [ERPL_SUMMARY_DIM][n]
  const int32_t* status;   // [n] or NULL
  uint8_t* why;            // [n] workspace: reason bits of every sample
  uint8_t* reasons;        // [n] caller's copy of the same, or NULL
  ErplAnaWork* work;
  int64_t n;
  double max_apogee, min_apogee, max_range, max_flight_time, energy_apogee;
  int32_t n_rows, n_q;
  int32_t rows[ERPL_ANALYSIS_MAX_ROWS];
  double q[ERPL_ANALYSIS_MAX_Q];
};
extern "C++" {
// Enqueues every pass of erpl_mc_analyze on `stream`; afterwards a.work->res holds the device's part of the result.
// Returns a hipError_t (0 = launched).
int erpl_launch_analysis(const ErplAnaArgs& a, void* stream);
// The moment passes and the selection of erpl_launch_analysis WITHOUT classify, for a caller that brings its own mask:
// a.why is read, never written (a byte of 0 = the sample counts), a.status / a.reasons and the bounds are not looked at.
// erpl_mc_dispersion describes its derived miss-distance row with it (a.summary = that row, a.rows[0] = 0, a.n_rows = 1).
// Afterwards a.work->res.row[] is filled; res.counter[] is left alone.
int erpl_launch_row_stats(const ErplAnaArgs& a, void* stream);
}

// ---- erpl_mc_histogram / erpl_mc_histogram_xy / erpl_mc_dispersion (erpl_distributions.hip) ----
// Grids are those of the analysis passes: min(ERPL_ANA_MAX_BLOCKS, ceil(n / ERPL_ANA_BLOCK)) workgroups of ERPL_ANA_BLOCK.
#define ERPL_DIST_TILE_CELLS 4096   // 2-D grids up to this many cells are counted in an LDS tile (16 KB of 32-bit counts),
                                    //   larger ones straight into the 64-bit global cells
struct ErplDistRange {              // finished by erpl_dist_finish_range, read by the host
  double lo[ERPL_HIST_MAX_ROWS], hi[ERPL_HIST_MAX_ROWS];
};
struct ErplDistHist {               // the 1-D result block the host copies back
  unsigned long long counted[ERPL_HIST_MAX_ROWS], below[ERPL_HIST_MAX_ROWS], above[ERPL_HIST_MAX_ROWS];
  unsigned long long bins[ERPL_HIST_MAX_ROWS][ERPL_HIST_MAX_BINS];
};
struct ErplDistMoments {            // dispersion: what the device hands back
  unsigned long long count;
  double mean_x, mean_y, sxx, sxy, syy;   // sums of dx dx, dx dy, dy dy about the mean
  double cov_xx, cov_xy, cov_yy, det;
  double centre_x, centre_y;
  unsigned long long inside[ERPL_DISP_MAX_LEVELS];
};
struct ErplDistWork {
  double pmin[ERPL_HIST_MAX_ROWS][ERPL_ANA_MAX_BLOCKS];      // range pass: partials per row and workgroup
  double pmax[ERPL_HIST_MAX_ROWS][ERPL_ANA_MAX_BLOCKS];
  ErplDistRange range;
  double edges[ERPL_HIST_MAX_ROWS][ERPL_HIST_MAX_BINS + 1];  // written by the host (2-D: lines 0 and 1 are x and y)
  ErplDistHist hist;
  unsigned long long counted2, outside2;
  unsigned long long cells[ERPL_HIST2D_MAX_BINS * ERPL_HIST2D_MAX_BINS];   // 2-D counts, x-major
  double dsum[3][ERPL_ANA_MAX_BLOCKS];                       // dispersion: partial sums per workgroup
  unsigned long long dcnt[ERPL_ANA_MAX_BLOCKS];
  unsigned long long ipart[ERPL_ANA_MAX_BLOCKS][ERPL_DISP_MAX_LEVELS];     // ellipse contents per workgroup
  ErplDistMoments mom;
};
struct ErplDistArgs {
  const double* summary;   // [ERPL_SUMMARY_DIM][n]
  const uint8_t* mask;     // [n] or NULL
  ErplDistWork* work;
  int64_t n;
  int32_t n_rows;
  int32_t rows[ERPL_HIST_MAX_ROWS];
  int32_t partner[ERPL_HIST_MAX_ROWS];   // range pass: a second row that has to be finite too (2-D), or -1
  int32_t bins[ERPL_HIST_MAX_ROWS];
  int32_t automatic[ERPL_HIST_MAX_ROWS]; // range pass: rows whose range comes from the data
  double lo[ERPL_HIST_MAX_ROWS], hi[ERPL_HIST_MAX_ROWS];   // bin passes: the range in use
};
struct ErplDispArgs {
  const double* summary;
  const uint8_t* mask;     // [n] or NULL
  ErplDistWork* work;
  double* miss;            // [n]: receives r, NaN where the sample is not counted
  int64_t n;
  int32_t row_x, row_y, centre, n_levels;
  double cx, cy;
  double k2[ERPL_DISP_MAX_LEVELS];
};
extern "C++" {
// Each enqueues its passes on `stream` and returns a hipError_t (0 = launched).
int erpl_launch_dist_range(const ErplDistArgs& a, void* stream);     // -> work->range
int erpl_launch_dist_hist(const ErplDistArgs& a, void* stream);      // work->edges -> work->hist
int erpl_launch_dist_hist2d(const ErplDistArgs& a, void* stream);    // work->edges[0..1] -> work->cells, counted2, outside2
int erpl_launch_dispersion(const ErplDispArgs& a, void* stream);     // -> work->mom, a.miss
}

// ---- erpl_mc_correlation (erpl_correlation.hip) ----
// The streaming passes use the grid of the analysis passes.  The Gram pass cuts the V x V matrix into 4 x 4 blocks
// (upper triangle: at most 78) and the samples into tiles of ERPL_CORR_TILE; workgroup w takes tiles w, w + grid, ...
// with grid = min(ERPL_CORR_GRAM_MAX_BLOCKS, ceil(n / ERPL_CORR_TILE)): functions of n and V alone.
#define ERPL_CORR_TILE 128
#define ERPL_CORR_GRAM_MAX_BLOCKS 512
#define ERPL_CORR_NB ((ERPL_CORR_MAX_VARS + 3) / 4)                       // 4 x 4 blocks per side
#define ERPL_CORR_GRAM_LEN (ERPL_CORR_NB * (ERPL_CORR_NB + 1) / 2 * 16)   // doubles of one blocked upper triangle
struct ErplCorrOut {                // what the device hands back
  unsigned long long counter[4];    // [0] population, [1] masked, [2] mask byte 0 but some variable not finite
  double mean[ERPL_CORR_MAX_VARS], vmin[ERPL_CORR_MAX_VARS], vmax[ERPL_CORR_MAX_VARS];
  double gram[2][ERPL_CORR_GRAM_LEN];   // centred cross-product sums, [0] of the values, [1] of the ranks; block (bi, bj),
                                        //   bi <= bj, at ((bi * (2 NB - bi + 1)) / 2 + bj - bi) * 16, element (p, q) at p * 4 + q
};
struct ErplCorrWork {
  ErplCorrOut out;
  double rank_mean[ERPL_CORR_MAX_VARS];   // (count + 1) / 2 for every variable: the mean of mid-ranks, exact
  double psum[ERPL_CORR_MAX_VARS][ERPL_ANA_MAX_BLOCKS];   // first moments: partials per variable and workgroup
  double pmin[ERPL_CORR_MAX_VARS][ERPL_ANA_MAX_BLOCKS];
  double pmax[ERPL_CORR_MAX_VARS][ERPL_ANA_MAX_BLOCKS];
  double gpart[ERPL_CORR_GRAM_MAX_BLOCKS][ERPL_CORR_GRAM_LEN];   // Gram: one blocked triangle per workgroup
};
struct ErplCorrArgs {
  const double* var[ERPL_CORR_MAX_VARS];   // [n] each: factor rows, then summary rows (or rows of ranks)
  const uint8_t* mask;                     // [n] or NULL
  uint8_t* pop;                            // [n] workspace: 0 = in the population, 1 = masked, 2 = not finite
  ErplCorrWork* work;
  int64_t n;
  int32_t n_vars;
};
extern "C++" {
// Each enqueues its passes on `stream` and returns a hipError_t (0 = launched).
int erpl_launch_corr_population(const ErplCorrArgs& a, void* stream);   // -> a.pop, work->out.counter / mean / vmin / vmax, rank_mean
int erpl_launch_corr_gram(const ErplCorrArgs& a, int which, void* stream);   // centred on out.mean (0) / rank_mean (1) -> out.gram[which]
// Mid-ranks of x within the population into rank_row (NaN outside it).  keys / idx: two [n] buffers each; temp: the sort's
// scratch of *temp_bytes.  With temp == NULL only *temp_bytes is set (nothing is enqueued).
int erpl_launch_corr_ranks(const ErplCorrArgs& a, const double* x, double* rank_row, unsigned long long* keys, uint32_t* idx,
                           void* temp, size_t* temp_bytes, void* stream);
}

// ---- erpl_mc_bootstrap (erpl_bootstrap.hip) ----
// Prepare works on the dense population (m members, in sample order): per requested row the values x[d], the same values
// ascending (sorted[p]) and the sorted position of every member (pos[d]).  The replicate kernel then needs 32-bit
// positions only: the k-th smallest position a replicate drew names its k-th order statistic.
struct ErplBootPrep {
  const double* var[ERPL_BOOT_MAX_ROWS];   // [n] each: the requested rows (summary rows or `extra`)
  const uint8_t* pop;                      // [n]: 0 = in the population (erpl_launch_corr_population)
  uint32_t* src;                           // [n]: the sample of dense member d
  unsigned long long* count;               // the select's own count of members (the host reads the population counter)
  double* x[ERPL_BOOT_MAX_ROWS];           // [m] each
  double* sorted[ERPL_BOOT_MAX_ROWS];      // [m] each
  uint32_t* pos[ERPL_BOOT_MAX_ROWS];       // [m] each
  unsigned long long* keys;                // [2 m] the sort's keys, in and out
  uint32_t* idx;                           // [2 m] the dense indices that travel with them
  void* temp;                              // scratch of the select and of the sort
  size_t temp_bytes;
  int64_t n, m;
  int32_t n_rows;
};
struct ErplBootArgs {
  const double* x[ERPL_BOOT_MAX_ROWS];
  const double* sorted[ERPL_BOOT_MAX_ROWS];
  const uint32_t* pos[ERPL_BOOT_MAX_ROWS];
  double* rep;                             // [n_rows * (2 + n_q)][replicates]: statistic s of replicate b at s * replicates + b
  unsigned long long seed;
  uint32_t m;                              // 1 .. 2^31 - 1
  int32_t n_rows, n_q, replicates;
  int32_t n_digits;                        // 8-bit digits that hold m - 1: 0 (m == 1) .. 4
  uint32_t rank[ERPL_ANA_TARGETS];         // targets 2 i and 2 i + 1: the ranks lo and hi behind quantile i, the same in
  double frac[ERPL_ANALYSIS_MAX_Q];        //   every replicate; frac[i] = pos - lo
};
extern "C++" {
// Each enqueues its passes on `stream` and returns a hipError_t (0 = launched).
// The scratch both rocPRIM calls of prepare need for n elements (nothing is enqueued).
int erpl_boot_temp_bytes(int64_t n, size_t* bytes);
// The scratch of the select alone (erpl_mc_sobol compacts its populations with erpl_launch_boot_compact and sorts nothing).
int erpl_boot_select_bytes(int64_t n, size_t* bytes);
int erpl_launch_boot_compact(const ErplBootPrep& p, void* stream);    // pop -> src, *count
int erpl_launch_boot_prepare(const ErplBootPrep& p, void* stream);    // src, var -> x, sorted, pos (p.m known)
int erpl_launch_boot_replicates(const ErplBootArgs& a, void* stream); // -> a.rep; one workgroup per replicate
}

// ---- erpl_mc_impact_density (erpl_density.hip) ----
// The streaming passes (moments, zones, fold, peak) use the grid of the analysis passes.  The pair kernel gives every
// thread ERPL_DENS_Q queries and stages the sources in LDS tiles of ERPL_DENS_TILE (16 KB of (u, v) pairs, read back at
// one address per wave: a broadcast); a workgroup owns ERPL_DENS_TILE queries and one slice of the sources.
#define ERPL_DENS_Q 4
#define ERPL_DENS_TILE (ERPL_DENS_Q * ERPL_ANA_BLOCK)   // 1024
#define ERPL_DENS_TARGET_BLOCKS 1024   // the sources are cut into slices until the launch has about this many workgroups
struct ErplDensMoments {            // what the moment passes hand back
  unsigned long long count;               // the select's
  double mean_x, mean_y, sxx, sxy, syy;   // sums of dx dx, dx dy, dy dy about the mean
  double min_x, max_x, min_y, max_y;      // +inf / -inf: nothing counted
};
struct ErplDensOut {                // what the zone pass and the finish hand back
  unsigned long long zone_inside[ERPL_DENSITY_MAX_ZONES];
  double sum, peak, peak_at;        // over the nodes; peak_at = the x-major index of the first node that holds the peak
};
struct ErplDensMap {                // a point of the plane -> whitened coordinates: u = w11 dx, v = fma(w21, dx, w22 dy)
  double mean_x, mean_y, w11, w21, w22;
};
struct ErplDensIn {                 // what the host writes: the nodes (np.linspace's arithmetic) and the zones of the spec
  double grid_x[ERPL_DENSITY_MAX_NODES], grid_y[ERPL_DENSITY_MAX_NODES];
  double zone_x[ERPL_DENSITY_MAX_VERTICES], zone_y[ERPL_DENSITY_MAX_VERTICES];
  int32_t zone_first[ERPL_DENSITY_MAX_ZONES + 1];
};
struct ErplDensWork {
  double psum[3][ERPL_ANA_MAX_BLOCKS];      // moments, node sum: partials per workgroup
  double pext[4][ERPL_ANA_MAX_BLOCKS];      // min x, max x, min y, max y; [0] also the peak and the peak's node
  unsigned long long zpart[ERPL_ANA_MAX_BLOCKS][ERPL_DENSITY_MAX_ZONES];   // zone contents per workgroup
  ErplDensMoments mom;
  ErplDensOut out;
  ErplDensIn in;
};
struct ErplDensArgs {
  const double* summary;   // [ERPL_SUMMARY_DIM][n]
  const uint8_t* mask;     // [n] or NULL
  ErplDensWork* work;
  uint8_t* pop;            // [n] workspace: 0 = counted (read by the select, the zones and the row statistics)
  int64_t n;
  int32_t row_x, row_y, n_zones;
};
// How the sources of a query are cut: `slices` runs of *per_slice consecutive dense indices (the last one shorter).  A
// function of m and the number of queries alone; the host sizes the partial sums with it and the launcher its grid.
inline int erpl_dens_slices(int64_t m, int64_t queries, int64_t* per_slice) {   // m, queries >= 1
  const int64_t t = (m + ERPL_DENS_TILE - 1) / ERPL_DENS_TILE, blocks = (queries + ERPL_DENS_TILE - 1) / ERPL_DENS_TILE;
  const int64_t want = (ERPL_DENS_TARGET_BLOCKS + blocks - 1) / blocks, most = t < want ? t : want;
  const int64_t tiles = (t + most - 1) / most;   // per slice, spread evenly
  *per_slice = tiles * ERPL_DENS_TILE;
  return (int)((t + tiles - 1) / tiles);
}
extern "C++" {
// Each enqueues its passes on `stream` and returns a hipError_t (0 = launched).
int erpl_launch_dens_population(const ErplDensArgs& a, void* stream);   // -> a.pop
// src[d] = the sample of dense member d < *count (the select's outputs, on the device): the counted points, in sample order,
// into xy[*count][2] and their moments, summed in an order that depends on them alone -> work->mom
int erpl_launch_dens_moments(const ErplDensArgs& a, const uint32_t* src, const unsigned long long* count, double* xy,
                             void* stream);
int erpl_launch_dens_zones(const ErplDensArgs& a, void* stream);     // a.pop, work->in -> work->out.zone_inside
int erpl_launch_dens_whiten(double* xy, int64_t m, const ErplDensMap& map, void* stream);   // xy[m][2] -> (u, v), in place
// the nodes of work->in.grid_x x work->in.grid_y, x-major, into whitened coordinates uv[nx * ny][2]
int erpl_launch_dens_nodes(const ErplDensWork* work, int nx, int ny, const ErplDensMap& map, double* uv, void* stream);
// THE pair kernel and its fold: out[scatter ? scatter[q] : q] = norm * sum over the m sources of exp(-|qry[q] - src[i]|^2 / 2)
// in the order of erpl_dens_slices; partial: erpl_dens_slices(m, queries) * queries doubles
int erpl_launch_dens_pairs(const double* qry, int64_t queries, const double* src, int64_t m, double norm, double* partial,
                           double* out, const uint32_t* scatter, void* stream);
int erpl_launch_dens_peak(ErplDensWork* work, const double* density, int64_t nodes, void* stream);   // -> work->out.sum / peak / peak_at
int erpl_launch_dens_fill_nan(double* row, int64_t n, void* stream);
// the fold of erpl_launch_dens_pairs on its own: the weighted pair kernel (erpl_launch_densw_pairs) leaves its slices to it
int erpl_launch_dens_fold(const double* partial, int slices, int64_t queries, double norm, double* out, const uint32_t* scatter,
                          void* stream);
}

// ---- erpl_mc_impact_density_weighted (erpl_density_w.hip) ----
// The passes of erpl_density.hip with an integer weight per sample.  Whiten, nodes, fold, peak and fill_nan are THE launchers
// above, run on `d`; the population, the moments, the zones and the selection are the unit's own.  The pair kernel is the
// weighted instantiation of erpl_dens_pairs (erpl_density.hip), with (u, v, w) per source in its LDS tile (24 KB).
struct ErplDensWMoments {           // what the population and the moment passes hand back
  unsigned long long count, n_masked, n_non_finite, n_zero, sum_w, max_w;
  double first_bad;                       // the lowest column whose weight is outside 0 .. 2^Q (+inf: none)
  int32_t K, reserved;                    // the bit length of max_w: w = W 2^-K
  double s_d, sum_w2;                     // sum_w 2^-K, sum w w
  double mean_x, mean_y, sxx, sxy, syy;   // sums of w dx dx, w dx dy, w dy dy about the mean
  double min_x, max_x, min_y, max_y;      // +inf / -inf: nothing counted
};
struct ErplDensWOut {               // what the zone pass and the selection hand back
  unsigned long long zone_w[ERPL_DENSITY_MAX_ZONES];
  double zone_a2[ERPL_DENSITY_MAX_ZONES];
  unsigned long long key[ERPL_DENSITY_MAX_LEVELS];        // key_of_signed of the thresholds
  unsigned long long content_w[ERPL_DENSITY_MAX_LEVELS];
  double f_min, f_max;
};
typedef ErplSelect<ERPL_DENSITY_MAX_LEVELS> ErplDensWSelect;   // the weighted radix selection, one target per level
struct ErplDensWWork {
  ErplDensWork d;                   // the block of the launchers of erpl_density.hip: in, out.sum / peak / peak_at, psum, pext
  unsigned long long pcnt[ERPL_ANA_MAX_BLOCKS][4];        // population: masked, non-finite, zero, counted per workgroup
  unsigned long long psum_w[ERPL_ANA_MAX_BLOCKS];
  double pmax_w[ERPL_ANA_MAX_BLOCKS], pbad[ERPL_ANA_MAX_BLOCKS];
  double za2[ERPL_ANA_MAX_BLOCKS][ERPL_DENSITY_MAX_ZONES];                  // zone sums of w w per workgroup (zone_w: d.zpart)
  unsigned long long cpart[ERPL_ANA_MAX_BLOCKS][ERPL_DENSITY_MAX_LEVELS];   // contents per workgroup
  unsigned long long hist[ERPL_DENSITY_MAX_LEVELS][ERPL_ANA_BINS];          // 64-bit digit histograms of the selection
  ErplDensWSelect sel;
  ErplDensWMoments mom;
  ErplDensWOut out;
};
struct ErplDensWArgs {
  const double* summary;   // [ERPL_SUMMARY_DIM][n]
  const uint8_t* mask;     // [n] or NULL
  const int64_t* weights;  // [n]
  ErplDensWWork* work;
  uint8_t* pop;            // [n] workspace: 0 = counted
  int64_t n;
  int32_t row_x, row_y, n_zones, Q;   // Q: a weight is admitted in 0 .. 2^Q
};
extern "C++" {
// Each enqueues its passes on `stream` and returns a hipError_t (0 = launched).
int erpl_launch_densw_population(const ErplDensWArgs& a, void* stream);   // -> a.pop, work->mom (counts, sum_w, max_w, K, s_d, first_bad)
// src[d] = the sample of dense member d < *count: the counted points into xy[*count][2], their scaled weights into ws[*count],
// and the weighted moments -> work->mom
int erpl_launch_densw_moments(const ErplDensWArgs& a, const uint32_t* src, const unsigned long long* count, double* xy, double* ws,
                              void* stream);
// over the dense points BEFORE they are whitened: work->d.in -> work->out.zone_w / zone_a2
int erpl_launch_densw_zones(const ErplDensWArgs& a, const double* xy, const double* ws, int64_t m, void* stream);
// THE weighted pair kernel: partial[slice][q] = sum over the slice's sources of w exp(-|qry[q] - src[i]|^2 / 2), in index order;
// the slices are erpl_dens_slices(m, queries) and erpl_launch_dens_fold adds them
int erpl_launch_densw_pairs(const double* qry, int64_t queries, const double* src, const double* ws, int64_t m, double* partial,
                            void* stream);
// the weighted selection over row[n] (the f_j; a.pop, a.weights) for n_levels targets, rank[k] = T_k - 1 (0-based, from the
// host: it knows sum_w), then the contents and the extremes -> work->out.key / content_w / f_min / f_max
int erpl_launch_densw_regions(const ErplDensWArgs& a, const double* row, const unsigned long long* rank, int n_levels, void* stream);
}

// ---- erpl_mc_corridor_resample / erpl_mc_corridor_bands (erpl_corridor.hip) ----
// Both kernels use workgroups of ERPL_ANA_BLOCK threads: one per trajectory (resample), one per row (c, k) of the matrix
// (bands).  The bands kernel hands back one ErplAnaRow per row - what the passes of erpl_mc_analyze hand back for a row of
// a summary, so the host finishes both the same way - and one more record behind them whose `count` is the number of
// columns with mask byte 0.
struct ErplCorridorResampleArgs {
  const double* traj;        // [n_traj][traj_cap][ERPL_TRAJ_DIM]
  const int64_t* traj_len;   // [n_traj]
  double* values;            // [n_channels][n_nodes][ld]
  int64_t n_traj, traj_cap, ld, col0;
  int32_t n_channels, n_nodes, hold;
  int32_t channels[ERPL_CORRIDOR_MAX_CHANNELS];
  double t0, dt;
};
struct ErplCorridorBandsArgs {
  const double* values;      // [rows][ld]
  const uint8_t* mask;       // [m] or NULL
  ErplAnaRow* out;           // [rows + 1]
  int64_t m, ld;             // m < 2^31: the digit histograms are 32-bit LDS counters
  int32_t rows, n_q;
  double q[ERPL_ANALYSIS_MAX_Q];
};
extern "C++" {
// Each enqueues one kernel on `stream` and returns a hipError_t (0 = launched).
int erpl_launch_corridor_resample(const ErplCorridorResampleArgs& a, void* stream);   // 1 <= n_traj < 2^31
int erpl_launch_corridor_bands(const ErplCorridorBandsArgs& a, void* stream);
}

// ---- erpl_mc_corridor_depth (erpl_corridor_depth.hip) ----
// What the passes leave per channel, and everything the launches need: the caller's arrays and the pieces of erpl_depth_layout
// (erpl_depth.h) in the context's buffer.
struct ErplDepthChan {         // 64 bytes
  int64_t n_defined, n_central;
  unsigned long long n_outliers;
  int64_t median;
  double threshold, depth_max;
  int64_t spare[2];
};
struct ErplDepthArgs {
  const double* values;      // [n_channels][n_nodes][ld]
  const uint8_t* mask;       // [m] or NULL
  int64_t m, ld;
  int32_t n_channels, n_nodes;
  double central, factor;
  double *depth, *mei;       // the caller's [n_channels][m] arrays
  int32_t *nodes, *n_out, *first_out;
  uint8_t* central_flag;
  uint32_t* pair;            // [n_nodes][m][2]
  int32_t* rown;             // [n_nodes]
  unsigned long long* keys;  // [2][max(group, 1)][m]
  uint32_t* offs;            // [group + 1]
  void* temp;
  size_t temp_bytes;
  ErplDepthChan* chan;       // [n_channels]
  erpl_depth_row* rows;      // [n_channels n_nodes]
  unsigned long long* count; // [4]
  int32_t group, lds;        // erpl_depth_layout's
};
extern "C++" {
// the scratch the sorts of a call over m columns need, with `group` rows per group of the global path (0: the LDS path)
int erpl_depth_temp_bytes(int64_t m, int group, size_t* bytes);
// enqueues every pass on `stream` and returns a hipError_t (0 = launched)
int erpl_launch_depth(const ErplDepthArgs& a, void* stream);
}

// ---- erpl_mc_sobol (erpl_sobol.hip) ----
// Prepare compacts the population of every requested row into RECORDS: rec[r][d][0 .. k + 1] = the k + 2 block values
// (A, B, AB_0 .. AB_k-1) of dense member d of row r, contiguous.  A draw of the replicate kernel is then one contiguous
// read of (k + 2) * 8 bytes.  Sums are indexed like the statistics of a row: slot 0 the sum of yA and yB, 1 the sum of the
// centred squares, 2 + i the sum of (yB - f0) d_i, 2 + k + i the sum of d_i d_i.
#define ERPL_SOBOL_CHUNK 8                                    // factors whose sums a thread carries through one sweep
#define ERPL_SOBOL_SLOTS (2 + 2 * ERPL_SOBOL_MAX_FACTORS)     // 66
struct ErplSobolOut {               // the estimates: what the device hands back
  double f0[ERPL_SOBOL_MAX_ROWS];                      // slot 0 / (2 m)
  double sum[ERPL_SOBOL_MAX_ROWS][ERPL_SOBOL_SLOTS];
};
struct ErplSobolWork {
  ErplSobolOut out;
  double part[ERPL_SOBOL_MAX_ROWS][ERPL_SOBOL_SLOTS][ERPL_ANA_MAX_BLOCKS];   // partials per row, slot and workgroup
  ErplAnaRow bands[ERPL_SOBOL_MAX_STATS + 1];          // the summary over the replicates (erpl_launch_corridor_bands)
};
struct ErplSobolArgs {
  const double* var[ERPL_SOBOL_MAX_ROWS];   // block 0 of the requested row: block b, design row j at var[r][b * n_base + j]
  const uint32_t* src[ERPL_SOBOL_MAX_ROWS]; // [m[r]]: the design row of dense member d
  double* rec[ERPL_SOBOL_MAX_ROWS];         // [m[r]][k + 2]
  ErplSobolWork* work;
  double* rep;                              // [n_rows * (2 + 2 k)][replicates]: statistic s of replicate b at s * replicates + b
  unsigned long long seed;
  int64_t n_base;
  uint32_t m[ERPL_SOBOL_MAX_ROWS];          // (k + 2) * m < 2^31
  int32_t n_rows, k, replicates;
};
extern "C++" {
// Each enqueues its passes on `stream` and returns a hipError_t (0 = launched).
int erpl_launch_sobol_records(const ErplSobolArgs& a, void* stream);      // var, src -> rec
int erpl_launch_sobol_estimates(const ErplSobolArgs& a, void* stream);    // rec -> work->out
int erpl_launch_sobol_replicates(const ErplSobolArgs& a, void* stream);   // rec -> a.rep; one workgroup per (replicate, row)
}

// ---- erpl_mc_dependence (erpl_dependence.hip) ----
// Everything works on the dense population (m members, in sample order).  Per variable the (key_of_tied, dense index) pairs
// are sorted and every member gets its class byte from its mid-rank; a factor's class bytes lie at xc + f * x_stride, an
// outcome's cell bytes at yext + j * y_stride, EXTENDED: byte k holds the cell of member k mod m for every k < 2 m + 32, so
// that the table kernel reads the cells d + s .. d + s + 15 of a shifted pairing without a wrap.
struct ErplDepEst {                 // what the table of the run itself (no shift) hands back for one (row, factor)
  long long delta_num;
  int32_t classes_used, cells_used;
  double v[4];                      // delta, ks_max, ks_median, mi
};
struct ErplDepWork {
  ErplDepEst est[ERPL_DEP_MAX_ROWS * ERPL_DEP_MAX_FACTORS];   // pair (j, f) at j * n_factors + f
};
struct ErplDepArgs {
  const double* var[ERPL_DEP_MAX_FACTORS + ERPL_DEP_MAX_ROWS];   // [n] each: the factors, then the requested rows
  const uint32_t* src;              // [m]: the sample of dense member d (erpl_launch_boot_compact)
  double* yd[ERPL_DEP_MAX_ROWS];    // [m] each: the requested rows, dense
  uint8_t* xc;                      // [n_factors][x_stride]
  uint8_t* yext;                    // [n_rows][y_stride]
  unsigned long long* keys;         // [2 m] the sort's keys, in and out
  uint32_t* idx;                    // [2 m] the dense indices that travel with them
  void* temp;                       // scratch of the sort
  size_t temp_bytes;
  double* cstat;                    // [n_rows][n_factors][classes][6]: count, mean, sum (y - mean)^2, x_lo, x_hi, x_median
  long long* tab;                   // [n_rows][n_factors][classes][cells]
  double* null;                     // [n_rows][n_factors][4][shifts]
  ErplDepWork* work;
  unsigned long long seed;
  size_t x_stride, y_stride;        // multiples of 16 (erpl_dep_layout)
  uint32_t m;                       // 1 .. 2^31 - 1
  int32_t n_factors, n_rows, classes, cells, shifts;
};
extern "C++" {
// Each enqueues its passes on `stream` and returns a hipError_t (0 = launched).
int erpl_launch_dep_classes(const ErplDepArgs& a, void* stream);   // var, src -> yd, xc, yext, cstat
int erpl_launch_dep_tables(const ErplDepArgs& a, void* stream);    // xc, yext -> tab, work->est, null; one workgroup per table
}

// ---- erpl_mc_compare (erpl_compare.hip) ----
// Everything works on the POOLED dense members (N = m_a + m_b: A's in sample order, then B's).  Replicate q = 0 is the
// observed labelling ("identity": i < m_a), replicate q = p + 1 permutation p; the labels of 64 replicates of one member are
// one word of the bit matrix bits[i][word].  Permutations are processed in blocks of `wb` words so that the matrix stays
// below ERPL_CMP_BITS_MAX_BYTES: block k holds the words k wb .. k wb + wb - 1, and every pass below runs once per block.
#define ERPL_CMP_TILE 256               // members per workgroup of the pair pass = sources per LDS stage
#define ERPL_CMP_TARGET_BLOCKS 1024     // the sources are cut into slices until the pair launch has about this many workgroups
#define ERPL_CMP_MAX_CHUNKS 1024        // waves that share the walk along one sorted order, per word
#define ERPL_CMP_CHUNK_MIN 256          // sorted positions a wave walks at least
#define ERPL_CMP_BITS_MAX_BYTES ((size_t)256 << 20)
#define ERPL_CMP_PART_MAX_COLUMNS 16384 // chunks x words of a block: the chunk records stay below 64 MiB
struct ErplCmpRank {                    // one replicate of one row: exact integers
  long long k;                          // max |N c_A - m_a t| over the class ends (-1: none seen)
  long long at;                         // the first sorted position that reaches it
  long long sign;                       // of N c_A - m_a t there
  unsigned long long sum2r;             // sum of 2 r over side A
  unsigned long long sa_lo, sa_hi, sb_lo, sb_hi;   // sums of (2 r - 2 c)^2 over side A / side B, 128 bits each
};
inline int erpl_cmp_words(int P) { return (P + 1 + 63) / 64; }
inline int erpl_cmp_block_words(int64_t N, int P) {
  const int64_t W = erpl_cmp_words(P), fit = (int64_t)(ERPL_CMP_BITS_MAX_BYTES / 8) / (N > 0 ? N : 1);
  return (int)(fit < 1 ? 1 : (fit < W ? fit : W));
}
// how the sorted order of a row is cut: `chunks` runs of *len consecutive positions (the last one shorter)
inline int erpl_cmp_chunks(int64_t N, int wb, int64_t* len) {   // N >= 1
  int64_t most = ERPL_CMP_PART_MAX_COLUMNS / wb;
  if (most > ERPL_CMP_MAX_CHUNKS) most = ERPL_CMP_MAX_CHUNKS;
  int64_t want = (N + ERPL_CMP_CHUNK_MIN - 1) / ERPL_CMP_CHUNK_MIN;
  if (want > most) want = most;
  *len = (N + want - 1) / want;
  return (int)((N + *len - 1) / *len);
}
// how the sources of the pair pass are cut: `slices` runs of *per_slice consecutive pooled members (the last one shorter)
inline int erpl_cmp_slices(int64_t N, int wb, int64_t* per_slice) {   // N >= 1
  const int64_t tiles = (N + ERPL_CMP_TILE - 1) / ERPL_CMP_TILE;
  const int64_t want = (ERPL_CMP_TARGET_BLOCKS + tiles * wb - 1) / (tiles * wb), most = tiles < want ? tiles : want;
  const int64_t per = (tiles + most - 1) / most;   // stages per slice, spread evenly
  *per_slice = per * ERPL_CMP_TILE;
  return (int)((tiles + per - 1) / per);
}
struct ErplCmpArgs {
  const double* var_a[ERPL_CMP_MAX_ROWS + 2];   // [n_a] each: the requested rows, then x and y (bivariate)
  const double* var_b[ERPL_CMP_MAX_ROWS + 2];
  const uint32_t* src_a;                // [m_a]: the sample of A's dense member d (erpl_launch_boot_compact)
  const uint32_t* src_b;
  double* val[ERPL_CMP_MAX_ROWS];       // [N] each: the requested rows, pooled
  double* xy;                           // [N][2], bivariate
  unsigned long long* keys;             // [2 N] the sort's keys, in and out
  uint32_t* idx;                        // [2 N] the pooled indices that travel with them
  void* temp;                           // scratch of the sort
  size_t temp_bytes;
  uint32_t* sidx[ERPL_CMP_MAX_ROWS];    // [N] each: the pooled member at every sorted position
  unsigned long long* r2e[ERPL_CMP_MAX_ROWS];   // [N] each: 2 r of the position, bit 63: the last position of its tie class
  unsigned long long* thr;              // [words 64][2]: (key, index) of the m_a-th smallest pair of replicate q (q = 0 unused)
  unsigned long long* bits;             // [N][wb]
  uint32_t* cnt;                        // [chunks][wb 64]: A members per chunk, then their exclusive prefix over the chunks
  ErplCmpRank* part;                    // [chunks][wb 64]
  ErplCmpRank* rank;                    // [n_rows][words 64]
  double* at_value;                     // [n_rows]: the row value at rank[j][0].at
  double* epart;                        // [tiles slices][wb][64][3]: S_AA, S_AB, S_BB
  double* eout;                         // [words 64][3]
  unsigned long long seed;
  uint64_t N, m_a;                      // 1 <= m_a < N < 2^32
  int32_t n_rows, bivariate, permutations, words, wb;
};
extern "C++" {
// Each enqueues its passes on `stream` and returns a hipError_t (0 = launched).
int erpl_launch_cmp_prepare(const ErplCmpArgs& a, void* stream);           // src, var -> val, xy, sidx, r2e, thr
int erpl_launch_cmp_block(const ErplCmpArgs& a, int w0, int wl, void* stream);   // the words w0 .. w0 + wl - 1 -> rank, at_value, eout
}

// ---- erpl_mc_surrogate (erpl_surrogate.hip) ----
// The fitted members go through the passes ERPL_SUR_CHUNK at a time: Psi of a chunk is materialised as cols = P + n_rows rows
// (the terms, then the requested outcomes) of `ld` members, and A A^T of that matrix is summed per 128 x 128 tile of its
// upper triangle (pairs = tiles (tiles + 1) / 2) and per slice of the chunk's members.  The slices of a chunk and their
// length are functions of the chunk's length and of P alone (not of n_rows: the tiles are counted as if every row were
// requested); so is the order in which erpl_sur_fold adds the partials, and with it every bit of G and b.
#define ERPL_SUR_CHUNK 32768            // fitted members per chunk
#define ERPL_SUR_TILE 128               // rows / columns of an output tile: four waves with a 64 x 64 quarter each
#define ERPL_SUR_KT 16                  // members per LDS stage of the Gram kernel
#define ERPL_SUR_TARGET_BLOCKS 512      // a chunk is cut into slices until the Gram launch has about this many workgroups
#define ERPL_SUR_MIN_SLICE 256          // members a slice has at the least
#define ERPL_SUR_U_BYTES 65536          // LDS of the univariate values of a workgroup's samples (basis, predict)
inline int erpl_sur_tiles(int cols) { return (cols + ERPL_SUR_TILE - 1) / ERPL_SUR_TILE; }
inline int erpl_sur_pairs(int cols) { return erpl_sur_tiles(cols) * (erpl_sur_tiles(cols) + 1) / 2; }
// The most slices a chunk of at most `len` members of a P-term fit is cut into: what the partial tiles are sized by.  It
// grows with len, and erpl_sur_slices never returns more (its slice length is at least len over this number); the number
// of slices itself is NOT monotone in len - the rounding of the slice length to ERPL_SUR_KT can save slices of a longer chunk.
inline int erpl_sur_max_slices(int64_t len, int P) {
  int64_t s = ERPL_SUR_TARGET_BLOCKS / erpl_sur_pairs(P + ERPL_SUR_MAX_ROWS), most = (len + ERPL_SUR_MIN_SLICE - 1) / ERPL_SUR_MIN_SLICE;
  if (s > most) s = most;
  return (int)(s < 1 ? 1 : s);
}
// slices of a chunk of `len` members; *slice_len: members per slice, a multiple of ERPL_SUR_KT
inline int erpl_sur_slices(int64_t len, int P, int* slice_len) {
  const int64_t s = erpl_sur_max_slices(len, P);
  const int64_t per = ((len + s - 1) / s + ERPL_SUR_KT - 1) / ERPL_SUR_KT * ERPL_SUR_KT;
  *slice_len = (int)per;
  return (int)((len + per - 1) / per);
}
// samples (= threads) per workgroup of the basis and predict kernels: the largest power of two whose univariate values
// (n_vars degree doubles per sample) fit ERPL_SUR_U_BYTES, at most 256 and at least 16 (32 x 12 doubles: 21 samples fit)
inline int erpl_sur_group(int n_vars, int degree) {
  int t = 256;
  while (t > 16 && (size_t)t * (size_t)n_vars * (size_t)degree * 8 > ERPL_SUR_U_BYTES) t >>= 1;
  return t;
}
struct ErplSurWork {
  double part[ERPL_SUR_MAX_ROWS][4][ERPL_ANA_MAX_BLOCKS];   // the sums of a residual pass: partials per row, sum and workgroup
  double mean[ERPL_SUR_MAX_ROWS][2];                        // of the fitted / the held-out members
  double out[ERPL_SUR_MAX_ROWS][4];                         // tss_fit, rss_fit, tss_val, rss_val
};
