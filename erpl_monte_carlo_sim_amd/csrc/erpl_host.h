// erpl_host.h — what the host units of the C ABI share (erpl_api.hip, erpl_sampling.hip, erpl_stats_api.hip,
// erpl_legacy_device.hip, erpl_design.hip, erpl_qmc.hip, erpl_tally.hip, erpl_subset.hip, erpl_reweight.hip, erpl_casualty.hip, erpl_corridor_drivers.hip, erpl_corridor_w.hip): the error text behind erpl_mc_last_error, the context, and the host patterns that exist once.
// Internal, never installed.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <functional>
#include <thread>
#include <type_traits>
#include <vector>

#include "erpl_plan.h"
#include "erpl_stat_layout.h"
#include "erpl_tables.h"

// Formats the text erpl_mc_last_error returns and hands `code` back.  The thread-local buffer is defined once, in
// erpl_api.hip: a buffer per unit would leave the messages of the other units unread.
__attribute__((visibility("hidden"))) int erpl_fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return erpl_fail(ERPL_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// an int-returning call of this library: its code is handed on (the text is already in place)
#define ERPL_TRY(...)                    \
  do {                                   \
    const int rc_ = (__VA_ARGS__);       \
    if (rc_ != ERPL_OK) return rc_;      \
  } while (0)

// expr: the int an erpl_launch_* returns (0 or a hipError_t)
#define LAUNCH_TRY(expr, what)                                                                          \
  do {                                                                                                  \
    const int le_ = (expr);                                                                             \
    if (le_ != 0) return erpl_fail(ERPL_ERR_HIP, what ": %s", hipGetErrorString((hipError_t)le_));      \
  } while (0)
#define KERNEL_TRY(expr) LAUNCH_TRY(expr, "kernel launch failed")

// erpl_mc_histogram / _histogram_xy / _dispersion: pinned mirror of what the host reads and writes of ErplDistWork
struct DistHost {
  ErplDistRange range;
  double edges[ERPL_HIST_MAX_ROWS][ERPL_HIST_MAX_BINS + 1];
  ErplDistHist hist;
  unsigned long long counted2, outside2;
  unsigned long long cells[ERPL_HIST2D_MAX_BINS * ERPL_HIST2D_MAX_BINS];
  ErplDistMoments mom;
};

// erpl_mc_bootstrap: pinned copies of what its launches hand back - the population counters, the estimates (summary rows,
// `extra`) and the summary over the replicates in groups of ERPL_ANALYSIS_MAX_ROWS statistics
struct BootHost {
  unsigned long long counter[4];
  ErplAnaResult est[2];
  ErplAnaResult sum[(ERPL_BOOT_MAX_STATS + ERPL_ANALYSIS_MAX_ROWS - 1) / ERPL_ANALYSIS_MAX_ROWS];
};

// erpl_mc_impact_density: pinned mirror of what the host reads of ErplDensWork (moments, zone counts, peak) and writes
// to it (grid nodes, zone vertices)
struct DensHost {
  ErplDensMoments mom;
  ErplDensOut out;
  ErplDensIn in;
};

// erpl_mc_impact_density_weighted: the same mirror of ErplDensWWork
struct DensWHost {
  ErplDensWMoments mom;
  ErplDensWOut out;
  ErplDensOut peak;
  ErplDensIn in;
};

// erpl_mc_sobol: pinned copies of what its launches hand back - per row the population counters and the extremes of the
// blocks A and B (erpl_launch_corr_population), the sums of the estimates and the summary over the replicates
struct SobolHost {
  unsigned long long counter[ERPL_SOBOL_MAX_ROWS][4];
  double vmin[ERPL_SOBOL_MAX_ROWS][2], vmax[ERPL_SOBOL_MAX_ROWS][2];
  ErplSobolOut out;
  ErplAnaRow bands[ERPL_SOBOL_MAX_STATS + 1];
};

// erpl_mc_dependence: pinned copies of what its launches hand back - the population counters, the moments of the requested
// rows (summary rows, `extra`) and the record of every (row, factor) pair's own table
struct DepHost {
  unsigned long long counter[4];
  ErplAnaResult rows[2];
  ErplDepEst est[ERPL_DEP_MAX_ROWS * ERPL_DEP_MAX_FACTORS];
};

// erpl_mc_surrogate: pinned copies of what its launches hand back - the population counters and the sums of the residual passes
struct SurHost {
  unsigned long long counter[4];
  double out[ERPL_SUR_MAX_ROWS][4];
};

// erpl_mc_compare: pinned copies of what its launches hand back - per side the population counters and the moments and order
// statistics of the requested rows (summary rows, `extra`)
struct CmpHost {
  unsigned long long counter[2][4];
  ErplAnaResult rows[2][2];
};

// The only place a per-context device buffer grows (the policy of erpl_mc_reserve): never shrinks, freed by
// erpl_mc_destroy.  An earlier call on another stream may still read the old buffer, hence the device synchronise.
template <typename T>
int erpl_grow(T*& p, size_t& cap, size_t bytes) {
  if (bytes <= cap) return ERPL_OK;
  HIP_TRY(hipDeviceSynchronize());
  (void)hipFree(p);
  p = nullptr; cap = 0;
  HIP_TRY(hipMalloc((void**)&p, bytes));
  cap = bytes;
  return ERPL_OK;
}

// What the context keeps for one statistics unit: a fixed device block (Dev = void: none) and its pinned mirror, both
// allocated with the first call that needs them, and one device buffer that grows with the call (erpl_grow).
template <typename Dev, typename Host>
struct ErplStatUnit {
  Dev* work = nullptr;
  Host* host = nullptr;
  char* buf = nullptr;
  size_t cap = 0;                 // bytes, as every capacity erpl_grow keeps
  int first_use() {
    if constexpr (!std::is_void<Dev>::value)
      if (!work) HIP_TRY(hipMalloc((void**)&work, sizeof(Dev)));
    if (!host) HIP_TRY(hipHostMalloc((void**)&host, sizeof(Host), hipHostMallocDefault));
    return ERPL_OK;
  }
  int grow(size_t bytes) { return erpl_grow(buf, cap, bytes); }
  void release() {                // erpl_mc_destroy
    (void)hipFree(work); (void)hipFree(buf);
    if (host) (void)hipHostFree(host);
  }
};

// Slot 0 serves erpl_mc_run_batch (on the caller's stream); slots 0..depth-1 serve erpl_mc_submit_batch
// round-robin, each on its own internal stream.  Whoever uses a slot first waits (on the device) for
// the slot's previous batch and records `done` behind its own kernels.
#define ERPL_TICKET_RING 256
struct ErplSlot {
  void* res_r[2] = {nullptr, nullptr};      // resume-queue records (see erpl_tables.h)
  double* res_d[2] = {nullptr, nullptr};
  int32_t* res_i[2] = {nullptr, nullptr};
  unsigned long long* d_queue = nullptr;    // qcnt[ERPL_MAX_PHASES + 2], qhead[...], then the hand-over queue's two cursor arrays
  void* ext_r = nullptr;                    // hand-over queue records (fp64 throughput build -> reference-order kernel),
  double* ext_d = nullptr;                  //   allocated with the first ERPL_PREC_F64_FAST batch of the set
  int32_t* ext_i = nullptr;
  int64_t ext_cap = 0;
  unsigned long long* d_counters = nullptr; // 16 words
  int64_t cap = 0;
  hipEvent_t done = nullptr;                // everything of the slot's latest batch has run
  hipEvent_t main_done = nullptr;           // its main flight launch has (the sweep stream waits for this)
  bool used = false;                        // `done` has been recorded at least once
  unsigned long long* own_counters = nullptr; // pinned: d_counters[0..3] of the slot's latest erpl_mc_run_batch
  unsigned long long* h_counters = nullptr; // pinned host copy of d_counters[0..3] of the slot's latest batch: `own_counters`,
                                            // or the ticket record of the batch (erpl_mc_submit_batch)
  bool latest_is_run = false;               // the slot's latest batch came through erpl_mc_run_batch (no ticket record)
  int64_t last_n = 0, seq = 0;              // its size and its position in the order of all batches of the context
  ErplPlan last_plan;                       // how it was scheduled (erpl_mc_debug_counters words 6 and 7)
};

struct erpl_ctx {
  int device = 0;
  int n_cu = 256;
  bool has_cfg = false;
  ErplTables h_tables;            // host copy (scalars are passed to the kernels by value)
  ErplTables* d_tables = nullptr;
  // Two workspaces ("sets") per lane of erpl_mc_submit_batch, used alternately: slot[lane] and
  // slot[ERPL_MAX_OVERLAP + lane].  A batch with lane adoption runs its rail and main flight launch on the lane's
  // main stream and its sweep launches (the few long trajectories nobody adopted) on the lane's sweep stream, so
  // the lane's NEXT batch - on the other set - starts when the main launch is over and overlaps the sweeps:
  // batches of equal length submitted together run in step, and without this the tails of a whole round of
  // them met on an otherwise empty GPU before the next round could start.
  // Sweep streams and second sets exist only where the process has a hardware queue per stream or, at the HIP default
  // of four queues, where the sweep streams come from the other stream-priority pool (erpl_sweep_stream in erpl_plan.h);
  // otherwise the sweeps stay on the lane's main stream and the lane on its first set.
  ErplSlot slot[2 * ERPL_MAX_OVERLAP];
  hipStream_t lane_stream[ERPL_MAX_OVERLAP] = {};
  hipStream_t lane_sweep[ERPL_MAX_OVERLAP] = {};
  bool lane_sweep_pool[ERPL_MAX_OVERLAP] = {};   // lane_sweep[i] was created at the other pool's priority
  hipEvent_t lane_in_ready[ERPL_MAX_OVERLAP] = {};
  unsigned lane_uses[ERPL_MAX_OVERLAP] = {};   // batches the lane has taken: parity picks the set
  int64_t submitted = 0;          // tickets handed out
  // One record per ticket: its own completion event and its own pinned copy of the batch's counters, so
  // that erpl_mc_check_batch(T) waits for T alone and reports T's own lost records however often T's workspace has
  // been reused since.  A ring of the last ERPL_TICKET_RING tickets; a record that leaves the ring unreported is
  // latched in `recycled_incomplete`.
  hipEvent_t ring_done[ERPL_TICKET_RING] = {};
  int64_t ring_ticket[ERPL_TICKET_RING] = {};
  unsigned long long* ring_counters = nullptr;   // pinned [ERPL_TICKET_RING][4]
  int64_t acked = 0;                // tickets <= acked have been reported by a blocking check of ALL batches
  int64_t recycled_incomplete = 0;  // first incomplete ticket that left the ring before such a check saw it
  int last_slot = 0;              // slot of the most recent batch (erpl_mc_last_stats)
  int64_t reserve_n = 0;          // erpl_mc_reserve request, applied to a slot when it is first used
  int adopt_spin = 1 << 22;       // polls of an adopting lane for a claimed record's ready word (erpl_mc_set_adopt_spin)
  // The scheduling settings and history of the context, in the struct the policy reads (erpl_plan.h; its defaults are the
  // context's): depth (erpl_mc_create), adopt, sweep_pool, chunk, waves (their setters), seen_mean_steps.
  ErplSched sched;
  bool pool_on = false;           // the lanes take their sweep streams from the other priority pool (latched, erpl_sweep_stream)
  bool pool_known = false, pool_exists = false;   // hipDeviceGetStreamPriorityRange has been asked; it reports two priorities
  int pool_prio = 0;              //   the priority the pool streams are created at
  int short_depth = 4;            // erpl_mc_set_short_flight_overlap
  int64_t seen_seq = 0, batches = 0;
  // one wave per workgroup: a finished wave frees its slot for the next batch at once (measured 2-5 %
  // over 256-thread workgroups, alone and overlapped); refill as soon as a lane is idle (best: 1..4)
  int block = 64, max_blocks = 0, refill = 1;
  bool profiling = false;
  long long profiled_runs = 0;
  hipEvent_t ev[3 * ERPL_PROFILE_RING] = {};
  // The statistics units (ErplStatUnit above) and what grows in each.  erpl_mc_analyze: one reason byte per sample, also the
  // row of zero bytes that stands in for a mask.  erpl_mc_histogram / _histogram_xy / _dispersion: the miss distance, one
  // double per sample, when the caller keeps none.  erpl_mc_correlation, erpl_mc_bootstrap (no device block of its own: it
  // runs on those of `corr` and `ana`), erpl_mc_impact_density and erpl_mc_sobol: the pieces of erpl_stat_layout.h.
  ErplStatUnit<ErplAnaWork, ErplAnaResult> ana;
  ErplStatUnit<ErplDistWork, DistHost> dist;
  ErplStatUnit<ErplCorrWork, ErplCorrOut> corr;
  ErplStatUnit<void, BootHost> boot;
  ErplStatUnit<ErplDensWork, DensHost> dens;
  // erpl_mc_impact_density_weighted: the pieces of erpl_densw_layout in the buffer
  ErplStatUnit<ErplDensWWork, DensWHost> densw;
  // erpl_mc_corridor_bands: the row records its kernel hands back, nothing else (no fixed block, no pinned mirror)
  ErplStatUnit<void, char> corridor;
  // erpl_mc_sobol: the partial sums of its estimates and the row records of its summary in the fixed block, the pieces of
  // erpl_stat_layout.h in the buffer; its population pass runs on the block of `corr`
  ErplStatUnit<ErplSobolWork, SobolHost> sobol;
  // erpl_mc_dependence: the records of the pairs' own tables in the fixed block, the pieces of erpl_stat_layout.h in the
  // buffer; its population pass runs on the block of `corr`, its row moments on that of `ana`
  ErplStatUnit<ErplDepWork, DepHost> dep;
  // erpl_mc_compare: two buffers, both laid out by erpl_compare_layout - `cmp_pop` for the populations of the two runs, sized
  // by (n_a, n_b), and `cmp` for the pooled members, sized once the populations are counted; its population pass runs on
  // the block of `corr`, its row moments on that of `ana`
  ErplStatUnit<void, CmpHost> cmp;
  ErplStatUnit<void, char> cmp_pop;
  // erpl_mc_surrogate: the sums of its residual passes in the fixed block, the pieces of erpl_stat_layout.h in the buffer; its
  // population pass runs on the block of `corr`.  erpl_mc_surrogate_predict: the model it evaluates, nothing else
  ErplStatUnit<ErplSurWork, SurHost> sur;
  ErplStatUnit<void, char> sur_model;
  // the model on its way up: pinned, so that the copy of erpl_mc_surrogate_predict is asynchronous, and the event behind the
  // latest copy out of it (the next call waits for that copy alone before it writes the staging again)
  char* sur_pin = nullptr;
  size_t sur_pin_cap = 0;
  hipEvent_t sur_ev = nullptr;
  // erpl_mc_legacy_random_streams_device / _wind_profiles_device: one device buffer (flag, op tables, knot constants, the
  // MT19937 states of a tile and two sets of its accepted pairs) and its pinned staging (the tables on their way up, r2
  // down and f up, per set), both bounded by the tile; an event per set behind the tile's copy to the host
  char* legacy_buf = nullptr;
  size_t legacy_cap = 0;
  char* legacy_pin = nullptr;
  size_t legacy_pin_cap = 0;
  hipEvent_t legacy_ev[2] = {};
  // erpl_mc_design: the pinned word its kernel raises when a cycle walk is given up, and the event behind the latest call
  // (both made by the first call; erpl_design_check_flag reads them for the blocking checks)
  int* design_flag = nullptr;
  hipEvent_t design_ev = nullptr;
  // erpl_mc_qmc: the direction numbers V[ERPL_QMC_MAX_DIMS][32] on the device (128 KB, made by the first call); its pad rows
  // raise design_flag and its calls record design_ev, so the blocking checks cover them as they cover erpl_mc_design
  uint32_t* qmc_v = nullptr;
  // erpl_mc_tally_*: the device workspace of erpl_tally.hip (the spec, the candidate lists of the extremes) in the buffer, the
  // spec that is on the device in the pinned mirror
  ErplStatUnit<void, erpl_tally_spec> tally;
  // erpl_mc_subset_*: the device workspace of erpl_subset.hip (the state of a selection, the rows' parameters of a proposal,
  // the tile counts of the compaction) in the buffer; the pinned staging of the parameters and the event behind its latest copy
  ErplStatUnit<void, char> subset;
  char* subset_pin = nullptr;
  hipEvent_t subset_ev = nullptr;
  // erpl_mc_reweight: the pieces of erpl_stat_layout.h in the buffer (the partials and the selection state of
  // erpl_reweight.hip, the log-weights and the weights the caller does not keep); the pinned copy of the sums it hands back
  ErplStatUnit<void, char> reweight;
  char* reweight_pin = nullptr;
  // erpl_mc_casualty: the pieces erpl_casualty.hip lists (its fixed block, the words of the map, the dense members of the groups,
  // the partials of the smoothing pass) in the buffer; what comes back is small or caller-sized and needs no pinned mirror
  ErplStatUnit<void, char> casualty;
  // erpl_mc_corridor_drivers: the pieces of erpl_cdrv_layout (erpl_stat_layout.h) in the buffer; what comes back is caller-sized
  // and needs no pinned mirror
  ErplStatUnit<void, char> cdrv;
  // erpl_mc_corridor_depth: the pieces of erpl_depth_layout (erpl_depth.h) in the buffer; what comes back is small or caller-sized
  ErplStatUnit<void, char> depth;
  // erpl_mc_corridor_bands_weighted: the slots of its first pass and a record per row (erpl_corridor_w.hip)
  ErplStatUnit<void, char> bands_w;
};

// erpl_design.hip
__attribute__((visibility("hidden"))) int erpl_design_check_flag(erpl_ctx* c);
__attribute__((visibility("hidden"))) int erpl_design_flag_init(erpl_ctx* c);

// The scale of an accepted pair of the legacy polar Gaussian (LegacyRS::next_gauss, and the host phase of the device
// streams): the one copy, so that both go through the same libm log with the same rounding of the quotient.
inline double legacy_gauss_scale(double r2) { return sqrt(-2.0 * log(r2) / r2); }

// The host pools: worker w of nthr takes the samples [n * w / nthr, n * (w + 1) / nthr) or every nthr-th table entry.
inline int host_threads(int32_t requested, int64_t n) {
  int nthr = requested > 0 ? requested : (int)std::thread::hardware_concurrency();
  if (nthr < 1) nthr = 1;
  if (requested <= 0 && nthr > 32) nthr = 32;   // containers often expose more cores than their quota
  if ((int64_t)nthr * 64 > n) nthr = (int)((n + 63) / 64);   // at least 64 samples per thread
  return nthr < 1 ? 1 : nthr;
}
inline void run_threads(int nthr, const std::function<void(int)>& work) {
  if (nthr == 1) { work(0); return; }
  std::vector<std::thread> pool;
  for (int w = 0; w < nthr; ++w) pool.emplace_back(work, w);
  for (auto& t : pool) t.join();
}
