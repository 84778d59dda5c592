// erpl_analysis.hip — the device passes of erpl_mc_analyze: outlier filter, moments and exact order statistics of the
// per-sample summary, replacing _filter_physics_outliers + _analyze_results of the reference (monte_carlo.py:337-473).
//
// Every pass streams rows of the [16][n] summary once, coalesced, on a grid that is a function of n alone:
//   classify   reason byte of every sample from the three filter rows; counters per workgroup (no atomics)
//   moments    per described row: masked sum / count / min / max, then (x - mean)^2 with the mean read on the device
//   select     most-significant-digit radix selection of all order statistics of a row together: eight passes of one
//              8-bit digit histogram per group of targets that still share a key prefix (LDS integer atomics, flushed to
//              64-bit global bins), a small kernel between passes that fixes the next digit of every target
// Sums are accumulated per thread in index order and reduced in the fixed order of erpl_stat_device.h; integer adds
// commute.  So the result is the same bits in every call.  No floating-point atomics.  Compiled with -ffp-contract=off:
// (x - mean)^2 is rounded as np.std rounds it.
#include "erpl_stat_device.h"
#include "erpl_tally.h"

namespace {

// ---- classify: one sample per thread and iteration; the counts of a wave are ballots (uniform), the workgroup's go to
// its own slot of work->cpart
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_ana_classify(const ErplAnaArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ apo_p = a.summary + (int64_t)ERPL_SUM_APOGEE_ALT * n;
  const double* __restrict__ rng_p = a.summary + (int64_t)ERPL_SUM_RANGE * n;
  const double* __restrict__ ft_p = a.summary + (int64_t)ERPL_SUM_FLIGHT_TIME * n;
  const ErplFilter f = {a.max_apogee, a.min_apogee, a.max_range, a.max_flight_time, a.energy_apogee};
  unsigned long long cnt[ERPL_ANA_COUNTERS];
#pragma unroll
  for (int k = 0; k < ERPL_ANA_COUNTERS; ++k) cnt[k] = 0ull;
  // the loop bound is uniform over the wave: every lane takes part in every ballot
  for (int64_t base = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    const bool in = i < n;
    int why = 0, st = -1;
    if (in) {
      const double apo = apo_p[i], rng = rng_p[i], ft = ft_p[i];
      why = erpl_why_of(f, apo, rng, ft);   // the one definition of the reason bits (erpl_tally.h)
      a.why[i] = (uint8_t)why;
      if (a.reasons) a.reasons[i] = (uint8_t)why;
      if (a.status) st = a.status[i];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) cnt[k] += __popcll(__ballot(in && (why & (1 << k))));
    if (a.status) {
#pragma unroll
      for (int k = 0; k < 5; ++k) cnt[6 + k] += __popcll(__ballot(in && (st & 0xFF) == k));
      cnt[11] += __popcll(__ballot(in && (st & ERPL_ST_NAN)));
      cnt[12] += __popcll(__ballot(in && (st & ERPL_ST_INCOMPLETE)));
    }
    cnt[13] += __popcll(__ballot(in && why == 0));
  }
  const u64 s = counters_fold(cnt);
  if (threadIdx.x < ERPL_ANA_COUNTERS) a.work->cpart[blockIdx.x][threadIdx.x] = s;
}

// ---- moments.  SECOND = false: sum, count, min, max of the valid finite values of row rows[blockIdx.y];
// SECOND = true: sum of (x - mean)^2 with the mean of the first pass.
template <bool SECOND>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_ana_moments(const ErplAnaArgs a) {
  const int r = blockIdx.y;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.rows[r] * n;
  const uint8_t* __restrict__ why = a.why;
  const double mean = SECOND ? a.work->res.row[r].mean : 0.0;
  double sum = 0.0, mn = INFINITY, mx = -INFINITY;
  unsigned long long cnt = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < n; i += stride) {
    const double v = x[i];
    if (why[i] == 0 && finite_bits(v)) {
      if (SECOND) {
        const double d = v - mean;
        sum += d * d;
      } else {
        sum += v;
        ++cnt;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
      }
    }
  }
  if (SECOND) block_fold<Add>(sum);
  else block_fold<Add, Add, Min, Max>(sum, cnt, mn, mx);
  if (threadIdx.x == 0) {
    a.work->psum[r][blockIdx.x] = sum;
    if (!SECOND) { a.work->pcnt[r][blockIdx.x] = cnt; a.work->pmin[r][blockIdx.x] = mn; a.work->pmax[r][blockIdx.x] = mx; }
  }
}

// ---- after the first moment pass: workgroup r < n_rows finishes row r and sets up its selection; workgroup n_rows adds
// up the classify counters
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_ana_finish_first(const ErplAnaArgs a, const int nb) {
  __shared__ unsigned long long s_cnt[ERPL_ANA_BLOCK];
  ErplAnaWork* w = a.work;
  if ((int)blockIdx.x == a.n_rows) {
    // thread = (slice of 64 workgroups, counter)
    const int c = threadIdx.x % ERPL_ANA_COUNTERS, slice = threadIdx.x / ERPL_ANA_COUNTERS;
    constexpr int slices = ERPL_ANA_BLOCK / ERPL_ANA_COUNTERS, per = ERPL_ANA_MAX_BLOCKS / slices;
    unsigned long long s = 0ull;
    for (int k = 0; k < per; ++k) { const int j = slice * per + k; if (j < nb) s += w->cpart[j][c]; }
    s_cnt[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < ERPL_ANA_COUNTERS) {
      for (int k = 1; k < slices; ++k) s += s_cnt[k * ERPL_ANA_COUNTERS + threadIdx.x];
      w->res.counter[threadIdx.x] = s;
    }
    return;
  }
  const int r = blockIdx.x;
  double sum = thread_partials<Add>(w->psum[r], nb);
  u64 cnt = thread_partials<Add>(w->pcnt[r], nb);
  double mn = thread_partials<Min>(w->pmin[r], nb), mx = thread_partials<Max>(w->pmax[r], nb);
  block_fold<Add, Add, Min, Max>(sum, cnt, mn, mx);
  if (threadIdx.x == 0) {
    ErplAnaRow& o = w->res.row[r];
    o.count = cnt; o.sum = sum; o.vmin = mn; o.vmax = mx; o.m2 = 0.0;
    o.mean = sum / (double)cnt;   // NaN for an empty row; the host reports every double of such a row as NaN
    // ranks of the two order statistics behind every quantile (np.percentile, linear)
    for (int t = 0; t < ERPL_ANA_TARGETS; ++t)
      select_start(w->sel[r], o.key, t, cnt > 0ull && t < 2 * a.n_q ? select_rank(cnt, a.q[t >> 1], t) : 0ull);
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_ana_finish_second(const ErplAnaArgs a, const int nb) {
  double m2 = thread_partials<Add>(a.work->psum[blockIdx.x], nb);
  block_fold<Add>(m2);
  if (threadIdx.x == 0) a.work->res.row[blockIdx.x].m2 = m2;
}

// ---- the selection (select_pass / select_step of erpl_stat_device.h): a digit pass over row rows[blockIdx.y], where a
// valid finite value counts once; between the passes workgroup r settles the digit for row r
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_ana_histogram(const ErplAnaArgs a, const int shift) {
  const int r = blockIdx.y;
  const int64_t n = a.n;
  const double* __restrict__ x = a.summary + (int64_t)a.rows[r] * n;
  const uint8_t* __restrict__ why = a.why;
  select_pass<unsigned int>(a.work->sel[r], a.work->hist[r], 2 * a.n_q, n, shift, [=](int64_t i, u64* key, unsigned int*) {
    const double v = x[i];
    *key = key_of_signed(v);
    return why[i] == 0 && finite_bits(v);
  });
}

__global__ __launch_bounds__(64 * ERPL_ANA_TARGETS) void erpl_ana_scan(const ErplAnaArgs a, const int shift) {
  const int r = blockIdx.x;
  select_step(a.work->sel[r], a.work->hist[r], a.work->res.row[r].key, 2 * a.n_q, shift);
}

}  // namespace

// moments, finish, moments, finish, eight selection passes; with `classify` the outlier filter in front of them and one
// more workgroup in the first finish, which adds up its counters (without it: n_rows > 0)
static int launch_passes(const ErplAnaArgs& a, const bool classify, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);
  hipError_t e = hipMemsetAsync(&a.work->hist[0][0][0], 0, sizeof(a.work->hist), st);
  if (e != hipSuccess) return (int)e;
  if (classify) hipLaunchKernelGGL(erpl_ana_classify, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a);
  if (a.n_rows > 0) hipLaunchKernelGGL(erpl_ana_moments<false>, dim3(nb, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(erpl_ana_finish_first, dim3(a.n_rows + (classify ? 1 : 0)), dim3(ERPL_ANA_BLOCK), 0, st, a, nb);
  if (a.n_rows > 0) {
    hipLaunchKernelGGL(erpl_ana_moments<true>, dim3(nb, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a);
    hipLaunchKernelGGL(erpl_ana_finish_second, dim3(a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a, nb);
    if (a.n_q > 0)
      for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(erpl_ana_histogram, dim3(nb, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a, shift);
        hipLaunchKernelGGL(erpl_ana_scan, dim3(a.n_rows), dim3(64 * ERPL_ANA_TARGETS), 0, st, a, shift);
      }
  }
  return (int)hipGetLastError();
}

int erpl_launch_analysis(const ErplAnaArgs& a, void* stream) { return launch_passes(a, true, stream); }

int erpl_launch_row_stats(const ErplAnaArgs& a, void* stream) { return a.n_rows > 0 ? launch_passes(a, false, stream) : 0; }
