// erpl_plan.h — how a batch is scheduled: how many lanes a context takes, which sweep stream a lane gets, and what
// erpl_mc_run_batch / erpl_mc_submit_batch launch for one batch.  Plain host C++ without HIP, environment or state of its
// own: erpl_api.hip hands in what it knows and wires up what comes back; csrc/erpl_plan_table.cpp prints the plans of
// tests/golden/plan_cases.json for tests/test_plan.py.  The measurements behind every rule: DESIGN.md section 3.2.
#pragma once
#include <math.h>
#include <stdint.h>

#include "erpl_tables.h"

// Lanes of a fresh context: two streams per lane (main, sweep) + the caller's stream and one more of its own; three with
// fewer than 12 hardware queues (the HIP default of four: the caller's stream + three lanes).
inline int erpl_default_depth(int queues) {
  return (queues >= 2 * ERPL_MAX_OVERLAP + 2) ? ERPL_MAX_OVERLAP : ((queues >= 12) ? (queues - 2) / 2 : 3);
}

// ---- the lane's sweep stream --------------------------------------------------------------------------------------
// The pool streams and the second workspaces (448 bytes per sample each) come with the first batch of at least this size:
// the smallest size measured, and it paid at every size tried - what a lane waits for is its own batch's few long
// trajectories, not a free SIMD.  Batches up to 8 192 samples were not measured and stay as they were: one stream per
// lane, nothing more allocated.
constexpr int64_t kSweepPoolMinBatch = 9216;
// ... and only for the fp64 throughput build: fp32 and the gate were not measured with pool streams and stay on the
// lane's one stream (erpl_mc_reserve asks for this build: the second workspaces are there when such a batch comes).
constexpr int kSweepPoolPrecision = ERPL_PREC_F64_FAST;

// NONE: the lane keeps to its one stream and one workspace, with or without lane adoption.  OWN: a second stream of the
// default priority - the process has a hardware queue for it.  POOL: a second stream from the other stream-priority pool.
enum ErplSweepKind { ERPL_SWEEP_NONE = 0, ERPL_SWEEP_OWN = 1, ERPL_SWEEP_POOL = 2 };

// The scheduling settings and history of a context (erpl_ctx::sched: these defaults are the context's).
struct ErplSched {
  int depth = 3;                // lanes erpl_mc_submit_batch cycles through (erpl_default_depth, erpl_mc_set_overlap)
  int adopt = -1;               // erpl_mc_set_adopt: the adoption limit; 0 = off; < 0 = by batch
  int sweep_pool = -1;          // erpl_mc_set_sweep_pool: -1 = from the first batch that fills the GPU, 0 = never, 1 = always
  int chunk = -1;               // erpl_mc_set_chunk: steps per launch between compactions; 0 = one launch; < 0 = by the batches seen
  int waves = 0;                // erpl_mc_set_waves_per_simd; 0 = by batch size
  double seen_mean_steps = 0.0; // physics RK4 steps per trajectory of the most recent batch the context has FINISHED
};

// What both decisions are told: those settings, the process and device, and the batch.  erpl_sweep_stream reads queues,
// depth, adopt, sweep_pool, precision and n; erpl_plan_batch everything but depth and sweep_pool.
struct ErplPlanIn : ErplSched {
  int queues = 4;               // hardware queues the process has
  int n_cu = 256;               // compute units of the device
  double max_time = 0.0, dt_flight = 0.005;   // horizon and flight step of the configuration
  int precision = kSweepPoolPrecision;   // of the batch (erpl_mc_reserve asks for the build that can take a pool stream)
  int64_t n = 0;                // samples submitted or reserved
  int64_t n_traj = 0;           // trajectories captured
  bool submit = false;          // erpl_mc_submit_batch (a ticket); false: erpl_mc_run_batch on the caller's one stream
  int in_flight = 1;            // lanes this submission goes round; 1 for erpl_mc_run_batch
  ErplSweepKind sweep = ERPL_SWEEP_NONE;   // what erpl_sweep_stream said for the batch (erpl_mc_run_batch: none)
  bool lane_stream_pool = false;           // the sweep stream the lane has was created at the other pool's priority
};

// Which sweep stream (and with it a second workspace) a lane takes for a batch of this size.
// - Own queue: lane adoption can come on and the process has a hardware queue for every stream - two per lane, the
//   caller's and one more of its own.
// - Other priority pool: the runtime keeps one pool of hardware queues PER STREAM PRIORITY, so a stream
//   created at another priority than the default shares no queue with the lanes' main streams or the caller's (a second
//   one of the default priority would land on another lane's queue, where the hand-overs cost more than they save).
//   For the build of kSweepPoolPrecision only; not from 12 queues up (those processes stay as they were); not where the
//   lanes' main streams share queues among themselves already (more lanes than queues besides the caller's); not on a
//   device that reports a single stream priority.
// pool_on is the context's latch: once the lanes take pool streams they go on doing so (the workspaces are there) until
// erpl_mc_set_sweep_pool(0).  two_priorities() answers whether the device reports two stream priorities
// (hipDeviceGetStreamPriorityRange, kept in erpl_api.hip); it is asked only where the latch is about to be set.
template <typename TwoPriorities>
ErplSweepKind erpl_sweep_stream(const ErplPlanIn& in, bool& pool_on, TwoPriorities&& two_priorities) {
  if (in.adopt != 0 && in.queues >= 2 * in.depth + 2) return ERPL_SWEEP_OWN;
  if (in.precision != kSweepPoolPrecision || in.adopt == 0 || in.sweep_pool == 0) return ERPL_SWEEP_NONE;
  if (in.queues >= 12 || in.depth + 1 > in.queues) return ERPL_SWEEP_NONE;
  if (!pool_on && (in.sweep_pool > 0 || in.n >= kSweepPoolMinBatch)) pool_on = two_priorities();
  return pool_on ? ERPL_SWEEP_POOL : ERPL_SWEEP_NONE;
}

// ---- one batch ----------------------------------------------------------------------------------------------------
// Trajectory length is not known in advance: the choices that depend on it (step chunks, how many batches of short
// flights start side by side) follow the batches the context has already FINISHED (seen_mean_steps).
constexpr double kLongFlightSteps = 8192.0;

struct ErplPlan {
  bool rotate_sets = false;     // the lane alternates its two workspaces
  int waves_per_simd = 2;
  int chunk_steps = 0;          // steps per flight launch between compactions; 0 = no step chunks
  int n_phases = 1;             // flight launches
  int adopt_lanes = 0;          // flying lanes at or below which a wave hands its lanes over; 0 = no lane adoption
  bool tail_on_sweep = false;   // the launches behind the main one go to the lane's sweep stream
  bool pool = false;            // that stream is from the other priority pool
  bool handoff = false;         // a hand-over sweep follows the last flight launch (the fp64 throughput build has one) ...
  int sweep_waves = 1;          // ... of this instantiation (erpl_launch_f64_sweep)
};

inline ErplPlan erpl_plan_batch(const ErplPlanIn& in) {
  ErplPlan p;
  const bool sweep = in.sweep != ERPL_SWEEP_NONE;
  // (a lane that got its stream under another setting keeps it: it counts as a pool stream only if it was created as one)
  p.pool = in.sweep == ERPL_SWEEP_POOL && in.lane_stream_pool;
  // two workspaces per lane only where the lane's next batch may start beside the sweeps of its previous one (a sweep
  // stream exists); erpl_mc_run_batch and lanes without one stay on their first set
  p.rotate_sets = sweep;
  // the three-wave build pays once three resident waves per SIMD stay busy: a batch that refills them a few times over
  // (between 1 and 3 rounds the rounding of "rounds" decides), or several batches in flight sharing the SIMDs
  const bool dense = in.n >= (int64_t)in.n_cu * 4 * 64 * 3 * 3 ||
                     (in.in_flight >= 2 && in.n * in.in_flight >= (int64_t)in.n_cu * 4 * 64 * 3);
  p.waves_per_simd = in.waves ? in.waves : (dense ? 3 : 2);
  // Step-chunked launches with compaction in between (erpl_mc_set_chunk).  Automatic (< 0, the default): compaction
  // pays when trajectories are long AND something else fills the GPU at every chunk barrier - overlapped batches of long
  // flights.  Results do not depend on the choice (bitwise).
  int chunk_steps = in.chunk;
  if (chunk_steps < 0) chunk_steps = (in.in_flight >= 2 && in.n_traj == 0 && in.seen_mean_steps >= kLongFlightSteps) ? 2048 : 0;
  // every lane ends within ceil(max_time / dt) + 1 steps, so that many steps' worth of chunks drains the queue
  if (chunk_steps > 0 && in.max_time > 0) {
    const double max_steps = ceil(in.max_time / in.dt_flight) + 2.0;
    double chunk = (double)chunk_steps;
    if (ceil(max_steps / chunk) + 1.0 > (double)ERPL_MAX_PHASES) chunk = ceil(max_steps / (double)(ERPL_MAX_PHASES - 2));
    p.chunk_steps = (int)chunk;
    p.n_phases = (int)ceil(max_steps / chunk) + 1;
  }
  // Lane adoption (erpl_mc_set_adopt): sweep launches behind the main one fly out what no running wave adopted.
  // Automatic (< 0, the default):
  // - On a sweep stream with a queue of its own the next batch of the lane follows the main launch at once and the few
  //   long trajectories of a batch finish beside it.  The one-wave-per-SIMD fp64 builds like the limit higher than fp32.
  //   (A lane whose stream has no queue of its own - fewer queues than two per lane in flight + 2 - goes without.)
  // - On a sweep stream from the other priority pool the lane runs as it does with a queue per stream: the limit of the
  //   sweep-stream case (a pool stream is handed in for the fp64 throughput build only).
  // - One stream per lane: submitted batches of the fp64 throughput build with two or more in flight to fill the SIMDs
  //   beside the sweeps, with the limit of the sweep-stream case; measured for that build only - fp32 and the gate stay
  //   as they were until they are measured there too.
  // - erpl_mc_run_batch runs on the caller's one stream with nothing beside it, where a batch is bound by its own longest
  //   trajectory and the hand-overs only lengthen that: off.
  // Step chunks already re-pack every lane, and chunk-parked records would be adopted straight back: exclusive.
  int adopt = in.adopt;
  if (adopt < 0 && sweep) adopt = p.pool ? 40 : ((in.queues >= 2 * in.in_flight + 2) ? (in.precision == ERPL_PREC_F32 ? 24 : 40) : 0);
  else if (adopt < 0) adopt = (in.submit && in.in_flight >= 2 && in.precision == ERPL_PREC_F64_FAST) ? 40 : 0;
  p.adopt_lanes = (in.n_traj == 0 && p.chunk_steps == 0) ? adopt : 0;
  // two sweeps behind the main launch, the first with adoption still on (it parks its own thin waves once more, the last
  // one never parks); ONE where they share the lane's only stream and the lane's next batch waits behind them
  const int adopt_phases = (in.submit && !sweep) ? 2 : 3;
  if (p.adopt_lanes > 0 && p.n_phases < adopt_phases) p.n_phases = adopt_phases;
  // with lane adoption the launches behind the main one hold the batch's few longest trajectories: they go to the
  // lane's sweep stream, and the lane's next batch (other set) follows the main launch at once
  p.tail_on_sweep = sweep && p.adopt_lanes > 0;
  // The hand-over sweep of the fp64 throughput build.  Where it runs on the stream that also carries the lane's next
  // batch (a submitted batch without a sweep stream, other batches filling the SIMDs meanwhile): the instantiation whose
  // waves start beside the throughput kernel's.  On a stream of its own, in erpl_mc_run_batch and for trajectory capture:
  // the gate's own (note [3] of erpl_k_config.h).  Not with step chunks: long flights were not measured in this mode and
  // keep the launch sequence they had.  On a stream from the other priority pool the capped one again: at four queues the
  // other lanes' main launches keep every SIMD busy, and the lane's set is free for its next batch but one only when the
  // sweep is over.
  const bool beside = in.submit && in.in_flight >= 2 && in.n_traj == 0 && p.chunk_steps == 0;
  p.handoff = in.precision == ERPL_PREC_F64_FAST;
  p.sweep_waves = (beside && (!sweep || p.pool)) ? 2 : 1;
  return p;
}

// erpl_mc_debug_counters word 7 (word 6 is adopt_lanes, the adoption limit of the batch's main launch): the instantiation
// of its hand-over sweep (0: the batch has none), + 16 with the sweeps on the lane's second stream, + 32 with that stream
// from the other pool.
inline int erpl_plan_word7(const ErplPlan& p) {
  return (p.handoff ? p.sweep_waves : 0) + (p.tail_on_sweep ? 16 : 0) + (p.tail_on_sweep && p.pool ? 32 : 0);
}
