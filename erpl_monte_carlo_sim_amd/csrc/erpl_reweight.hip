// erpl_reweight.hip — erpl_mc_reweight of the C ABI (include/erpl_mc.h): the statistics of a flown run under another input
// law, by integer importance weights.  The rule is erpl_reweight.h, here for the device (the kernels below) and for the host
// (erpl_mc_reweight_host); built without FMA contraction, so that a column's log-weight and the portable exp round alike on
// both and logw / weights are the same bits.
//
// The passes stream rows once, coalesced, on grid_of(n) workgroups; a thread accumulates its own columns in index order and
// the folds are those of erpl_stat_device.h, so the result is the same bits in every call.  Integer atomics only.
//   rw_logw            one column per thread and iteration: the law rows and the requested outcome rows read row by row,
//                      the column's state and log-weight; per workgroup the maximum of l and the counters (slots)
//   rw_finish_max      one workgroup: l_max and the counts
//   rw_weights         W of every column; per workgroup S, sum W^2, the zero weights, the heaviest
//   rw_finish_weights  one workgroup
//   rw_rows<false>     rows in blockIdx.y: sum W x, min, max, per threshold sum W [x > thr] and sum W^2 [x > thr]
//   rw_finish_rows     a workgroup per row: the mean, and the ranks of the order statistics
//   rw_rows<true>      sum W (x - mean)^2, sum W^2 (x - mean)^2 with the mean read on the device, and their finish
//   rw_hist / rw_scan  the radix selection of erpl_stat_device.h in its global-bin form, a column counting W times: eight
//                      passes of one 8-bit digit, 64-bit bins in LDS flushed to 64-bit global bins, a scan kernel between them
//                      (this unit's own copy of select_pass / select_step around the shared steps: see at the kernels)
// What binds them (DESIGN.md section 8.17 has the measurements, or says UNMEASURED): rw_logw reads 8 (n_law + rows) + 1 bytes
// per column and writes 8, every later pass reads 8 or 16 and the weights pass writes 8 - HBM bytes above some 10^6 columns,
// launch latency below (24 launches).
#include "erpl_host.h"

#include "erpl_reweight.h"
#include "erpl_stat_device.h"

namespace {
constexpr int kBlock = ERPL_ANA_BLOCK;          // 256: the folds of erpl_stat_device.h are written for it
constexpr int kMaxBlocks = ERPL_ANA_MAX_BLOCKS;
constexpr int kR = ERPL_RW_MAX_ROWS, kT = ERPL_RW_MAX_THRESHOLDS, kQ = ERPL_RW_MAX_Q;

typedef ErplSelect<kQ> RwSelect;

// the device workspace in front of the two column arrays (erpl_rw_layout): what the call hands back, the state of the
// selection, and a slot per workgroup for every partial
struct RwWork {
  ErplRwRaw raw;
  RwSelect sel[kR];
  u64 hist[kR][kQ][ERPL_ANA_BINS];
  double p_lmax[kMaxBlocks];
  u64 p_cnt[kMaxBlocks][4];
  u64 p_sum_w[kMaxBlocks], p_zero[kMaxBlocks];
  double p_sum_w2[kMaxBlocks], p_max_w[kMaxBlocks];
  double p_s0[kR][kMaxBlocks], p_s1[kR][kMaxBlocks];     // sum W x, then sum W d^2 | sum W^2 d^2
  double p_min[kR][kMaxBlocks], p_max[kR][kMaxBlocks];
  u64 p_exceed[kR][kT][kMaxBlocks];
  double p_a2[kR][kT][kMaxBlocks];
};

struct RwArgs {
  const double* factors;
  const double* summary;
  const double* extra;
  const uint8_t* mask;
  double* logw;
  int64_t* weights;
  RwWork* work;
  int64_t ld, ld_s, n;
  int32_t n_rows, n_q, Q, rows[kR], n_thr[kR];
  double thr[kR][kT], q[kQ];
};

// ---------------------------------------------------------------- log-weights and the population

__global__ __launch_bounds__(kBlock) void rw_logw(const RwArgs a, const ErplRwLaw law) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * kBlock;
  u64 cnt[4] = {0ull, 0ull, 0ull, 0ull};
  double lmax = -(double)INFINITY;
  // the loop bound is uniform over the wave: every lane takes part in every ballot
  for (int64_t base = (int64_t)blockIdx.x * kBlock + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    const bool in = i < n;
    int state = -1;
    if (in) {
      double l;
      state = erpl_rw_column(law, a.rows, a.n_rows, a.factors, a.ld, a.summary, a.ld_s, a.extra, a.mask, i, &l);
      a.logw[i] = l;
      if (state == ERPL_RW_IN) lmax = l > lmax ? l : lmax;
    }
    cnt[0] += (u64)__popcll(__ballot(state == ERPL_RW_MASKED));
    cnt[1] += (u64)__popcll(__ballot(state == ERPL_RW_NON_FINITE));
    cnt[2] += (u64)__popcll(__ballot(state == ERPL_RW_OUTSIDE));
    cnt[3] += (u64)__popcll(__ballot(state == ERPL_RW_IN));
  }
  block_fold<Max>(lmax);
  const u64 s = counters_fold(cnt);
  if (threadIdx.x == 0) a.work->p_lmax[blockIdx.x] = lmax;
  if (threadIdx.x < 4) a.work->p_cnt[blockIdx.x][threadIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void rw_finish_max(RwWork* w, const int nb) {
  double lmax = thread_partials<Max>(w->p_lmax, nb);
  u64 c0 = thread_partials<Add>(&w->p_cnt[0][0], nb, 4), c1 = thread_partials<Add>(&w->p_cnt[0][1], nb, 4);
  u64 c2 = thread_partials<Add>(&w->p_cnt[0][2], nb, 4), c3 = thread_partials<Add>(&w->p_cnt[0][3], nb, 4);
  block_fold<Max, Add, Add, Add, Add>(lmax, c0, c1, c2, c3);
  if (threadIdx.x == 0) {
    w->raw.lmax = lmax;
    w->raw.n_masked = c0; w->raw.n_non_finite = c1; w->raw.n_outside = c2; w->raw.count = c3;
  }
}

// ---------------------------------------------------------------- the weights

__global__ __launch_bounds__(kBlock) void rw_weights(const RwArgs a) {
  const int64_t n = a.n, stride = (int64_t)gridDim.x * kBlock;
  const double lmax = a.work->raw.lmax;
  u64 sum_w = 0ull, zero = 0ull;
  double sum_w2 = 0.0, max_w = -(double)INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const double l = a.logw[i];
    int64_t wi = 0;
    if (l > -(double)INFINITY) {
      wi = erpl_rw_weight(l, lmax, a.Q);
      const double wd = (double)wi;
      sum_w += (u64)wi;
      sum_w2 += wd * wd;
      zero += wi == 0 ? 1ull : 0ull;
      max_w = wd > max_w ? wd : max_w;
    }
    a.weights[i] = wi;
  }
  block_fold<Add, Add, Add, Max>(sum_w, zero, sum_w2, max_w);
  if (threadIdx.x == 0) {
    RwWork* w = a.work;
    w->p_sum_w[blockIdx.x] = sum_w; w->p_zero[blockIdx.x] = zero; w->p_sum_w2[blockIdx.x] = sum_w2; w->p_max_w[blockIdx.x] = max_w;
  }
}

__global__ __launch_bounds__(kBlock) void rw_finish_weights(RwWork* w, const int nb) {
  u64 sum_w = thread_partials<Add>(w->p_sum_w, nb), zero = thread_partials<Add>(w->p_zero, nb);
  double sum_w2 = thread_partials<Add>(w->p_sum_w2, nb), max_w = thread_partials<Max>(w->p_max_w, nb);
  block_fold<Add, Add, Add, Max>(sum_w, zero, sum_w2, max_w);
  if (threadIdx.x == 0) {
    w->raw.sum_w = sum_w; w->raw.n_zero = zero; w->raw.sum_w2 = sum_w2;
    w->raw.max_w = w->raw.count ? max_w : 0.0;
  }
}

// ---------------------------------------------------------------- the rows

// SECOND = false: sum W x, min, max over W > 0, and per threshold sum W [x > thr], sum W^2 [x > thr] of row rows[blockIdx.y];
// SECOND = true: sum W d^2 and sum W^2 d^2, d = x - mean with the mean of the first pass.
template <bool SECOND>
__global__ __launch_bounds__(kBlock) void rw_rows(const RwArgs a) {
  const int r = blockIdx.y, row = a.rows[r], n_thr = a.n_thr[r];
  const int64_t n = a.n, stride = (int64_t)gridDim.x * kBlock;
  const int64_t* __restrict__ wt = a.weights;
  RwWork* w = a.work;
  const double mean = SECOND ? w->raw.row[r].mean : 0.0;
  double s0 = 0.0, s1 = 0.0, mn = (double)INFINITY, mx = -(double)INFINITY;
  u64 ex[kT];
  double a2[kT], thr[kT];
#pragma unroll
  for (int k = 0; k < kT; ++k) { ex[k] = 0ull; a2[k] = 0.0; thr[k] = a.thr[r][k]; }
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t wi = wt[i];
    if (wi == 0) continue;
    const double v = erpl_rw_outcome(a.summary, a.ld_s, a.extra, row, i), wd = (double)wi;
    if (SECOND) {
      const double d = v - mean;
      const double dd = d * d;
      s0 += wd * dd;
      s1 += (wd * wd) * dd;
    } else {
      s0 += wd * v;
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
      const double w2 = wd * wd;
#pragma unroll
      for (int k = 0; k < kT; ++k)
        if (k < n_thr && v > thr[k]) { ex[k] += (u64)wi; a2[k] += w2; }
    }
  }
  if (SECOND) {
    block_fold<Add, Add>(s0, s1);
    if (threadIdx.x == 0) { w->p_s0[r][blockIdx.x] = s0; w->p_s1[r][blockIdx.x] = s1; }
  } else {
    block_fold<Add, Min, Max>(s0, mn, mx);
    if (threadIdx.x == 0) { w->p_s0[r][blockIdx.x] = s0; w->p_min[r][blockIdx.x] = mn; w->p_max[r][blockIdx.x] = mx; }
#pragma unroll
    for (int k = 0; k < kT; ++k) {
      if (k >= n_thr) break;                     // uniform over the workgroup
      block_fold_again<Add, Add>(ex[k], a2[k]);
      if (threadIdx.x == 0) { w->p_exceed[r][k][blockIdx.x] = ex[k]; w->p_a2[r][k][blockIdx.x] = a2[k]; }
    }
  }
}

// workgroup r finishes row r; after the first pass it also sets up the row's selection
template <bool SECOND>
__global__ __launch_bounds__(kBlock) void rw_finish_rows(const RwArgs a, const int nb) {
  const int r = blockIdx.x;
  RwWork* w = a.work;
  ErplRwRawRow& o = w->raw.row[r];
  if (SECOND) {
    double m2 = thread_partials<Add>(w->p_s0[r], nb), se2 = thread_partials<Add>(w->p_s1[r], nb);
    block_fold<Add, Add>(m2, se2);
    if (threadIdx.x == 0) { o.m2 = m2; o.se2 = se2; }
    return;
  }
  double sum = thread_partials<Add>(w->p_s0[r], nb), mn = thread_partials<Min>(w->p_min[r], nb), mx = thread_partials<Max>(w->p_max[r], nb);
  block_fold<Add, Min, Max>(sum, mn, mx);
  const u64 S = w->raw.sum_w;
  if (threadIdx.x == 0) {
    o.sum_wx = sum; o.vmin = mn; o.vmax = mx; o.m2 = 0.0; o.se2 = 0.0;
    o.mean = sum / (double)S;                    // NaN for an empty population: the host reports every double of it as NaN
    RwSelect& s = w->sel[r];
    for (int t = 0; t < kQ; ++t) {
      s.prefix[t] = 0ull; s.leader[t] = 0;
      s.rank[t] = S > 0ull && t < a.n_q ? erpl_rw_target(a.q[t], S) - 1ull : 0ull;
      o.key[t] = 0ull;
    }
  }
  for (int k = 0; k < a.n_thr[r]; ++k) {
    u64 ex = thread_partials<Add>(w->p_exceed[r][k], nb);
    double a2 = thread_partials<Add>(w->p_a2[r][k], nb);
    block_fold_again<Add, Add>(ex, a2);
    if (threadIdx.x == 0) { o.exceed[k] = ex; o.a2[k] = a2; }
  }
}

// ---------------------------------------------------------------- the weighted selection

// These two kernels are select_pass / select_step of erpl_stat_device.h written out: with the shared bodies the call at
// 131 072 columns measured 2.8 % slower than with these (profiles/select_refactor_ab.json), and no cause was found in the
// assembly, so they stay as they were.  A fix to the pass structure there has to be made here as well.

// One pass: per group of targets that still share a key prefix, the weight in every value of the digit at `shift` among the
// keys that match the prefix above it.  Only the first target of a group (its leader) keeps a histogram.
__global__ __launch_bounds__(kBlock) void rw_hist(const RwArgs a, const int shift) {
  __shared__ u64 s_hist[kQ][ERPL_ANA_BINS];      // 16 KB
  __shared__ u64 s_prefix[kQ];
  __shared__ int s_lead[kQ];
  __shared__ int s_nlead;
  const int r = blockIdx.y, row = a.rows[r];
  const int64_t n = a.n, stride = (int64_t)gridDim.x * kBlock;
  const int64_t* __restrict__ wt = a.weights;
  const RwSelect& sel = a.work->sel[r];
  for (int k = threadIdx.x; k < kQ * ERPL_ANA_BINS; k += kBlock) (&s_hist[0][0])[k] = 0ull;
  if (threadIdx.x == 0) {
    int m = 0;
    for (int t = 0; t < a.n_q; ++t)
      if (sel.leader[t] == t) { s_lead[m] = t; s_prefix[m] = sel.prefix[t]; ++m; }
    s_nlead = m;
  }
  __syncthreads();
  const int nlead = s_nlead;
  const int64_t first = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~63);
  for (int64_t base = first; base < n; base += stride) {   // uniform over the wave (ballots below)
    const int64_t i = base + (threadIdx.x & 63);
    u64 wi = 0ull, key = 0ull;
    if (i < n) {
      wi = (u64)wt[i];
      if (wi) key = key_of_signed(erpl_rw_outcome(a.summary, a.ld_s, a.extra, row, i));
    }
    select_count(s_hist, s_lead, s_prefix, nlead, wi != 0ull, key, shift, wi);
  }
  __syncthreads();
  for (int m = 0; m < nlead; ++m) {
    const int t = s_lead[m];
    for (int b = threadIdx.x; b < ERPL_ANA_BINS; b += kBlock) {
      const u64 c = s_hist[t][b];
      if (c) atomicAdd(&a.work->hist[r][t][b], c);
    }
  }
}

// Between the passes: wave t of workgroup r scans the histogram of target t's group, fixes the digit that holds its rank and
// reduces the rank to that bin; then the groups are formed again and the histograms are cleared.
__global__ __launch_bounds__(64 * kQ) void rw_scan(const RwArgs a, const int shift) {
  __shared__ u64 s_prefix[kQ];
  const int r = blockIdx.x, t = threadIdx.x >> 6, lane = threadIdx.x & 63, nt = a.n_q;
  RwSelect& sel = a.work->sel[r];
  if (t < nt) {
    const u64* h = a.work->hist[r][sel.leader[t]];
    const u64 rank = sel.rank[t];
    u64 prefix = sel.prefix[t], before = 0ull;
    int d = 0;
    if (lane == 0) s_prefix[t] = prefix;         // stays if no bin holds the rank: an empty population
    if (select_scan(h, rank, lane, &d, &before)) {   // exactly one lane
      prefix |= (u64)d << shift;
      sel.prefix[t] = prefix;
      sel.rank[t] = rank - before;
      a.work->raw.row[r].key[t] = prefix;
      s_prefix[t] = prefix;
    }
  }
  __syncthreads();   // every histogram has been read, every prefix is known
  if (lane == 0 && t < nt) sel.leader[t] = select_leader(s_prefix, t);
  u64* h = &a.work->hist[r][0][0];
  for (int k = threadIdx.x; k < kQ * ERPL_ANA_BINS; k += 64 * kQ) h[k] = 0ull;
}

// ---------------------------------------------------------------- the refusals, in the order of the header

constexpr int64_t kMostColumns = ((int64_t)1 << 31) - 1;

int reweight_check(const erpl_rw_spec* s, const double* factors, int64_t ld, const double* summary, int64_t ld_s, const double* extra,
                   int64_t n, const erpl_reweight* result) {
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (s->n_law < 1 || s->n_law > ERPL_RW_MAX_LAW) return erpl_fail(ERPL_ERR_INVALID, "n_law = %d outside 1 .. %d", s->n_law, ERPL_RW_MAX_LAW);
  for (int r = 0; r < s->n_law; ++r) {
    if (s->kind[r] == ERPL_DESIGN_NORMAL) {
      if (!erpl_is_finite(s->mu[r])) return erpl_fail(ERPL_ERR_INVALID, "mu[%d] = %g is not finite", r, s->mu[r]);
      if (!(erpl_is_finite(s->s[r]) && s->s[r] > 0.0)) return erpl_fail(ERPL_ERR_INVALID, "s[%d] = %g is not a finite positive number", r, s->s[r]);
    } else if (s->kind[r] == ERPL_DESIGN_UNIFORM) {
      if (!(s->a[r] >= 0.0 && s->a[r] < s->b[r] && s->b[r] <= 1.0))
        return erpl_fail(ERPL_ERR_INVALID, "a[%d], b[%d] = %g, %g outside 0 <= a < b <= 1", r, r, s->a[r], s->b[r]);
    } else {
      return erpl_fail(ERPL_ERR_INVALID, "kind[%d] = %d is neither ERPL_DESIGN_UNIFORM nor ERPL_DESIGN_NORMAL", r, (int)s->kind[r]);
    }
  }
  if (s->n_rows < 1 || s->n_rows > ERPL_RW_MAX_ROWS) return erpl_fail(ERPL_ERR_INVALID, "n_rows = %d outside 1 .. %d", s->n_rows, ERPL_RW_MAX_ROWS);
  for (int j = 0; j < s->n_rows; ++j)
    if (s->rows[j] < 0 || s->rows[j] > ERPL_RW_ROW_EXTRA) return erpl_fail(ERPL_ERR_INVALID, "rows[%d] = %d outside 0 .. %d", j, s->rows[j], ERPL_RW_ROW_EXTRA);
  for (int j = 0; j < s->n_rows; ++j)
    for (int k = 0; k < j; ++k)
      if (s->rows[j] == s->rows[k]) return erpl_fail(ERPL_ERR_INVALID, "rows[%d] = %d is listed twice", j, s->rows[j]);
  for (int j = 0; j < s->n_rows; ++j)
    if (s->rows[j] == ERPL_RW_ROW_EXTRA && !extra) return erpl_fail(ERPL_ERR_INVALID, "rows[%d] is ERPL_RW_ROW_EXTRA but extra is NULL", j);
  for (int j = 0; j < s->n_rows; ++j)
    if (s->n_thresholds[j] < 0 || s->n_thresholds[j] > ERPL_RW_MAX_THRESHOLDS)
      return erpl_fail(ERPL_ERR_INVALID, "n_thresholds[%d] = %d outside 0 .. %d", j, s->n_thresholds[j], ERPL_RW_MAX_THRESHOLDS);
  for (int j = 0; j < s->n_rows; ++j)
    for (int k = 0; k < s->n_thresholds[j]; ++k)
      if (s->threshold[j][k] != s->threshold[j][k]) return erpl_fail(ERPL_ERR_INVALID, "threshold[%d][%d] is NaN", j, k);
  if (s->n_q < 0 || s->n_q > ERPL_RW_MAX_Q) return erpl_fail(ERPL_ERR_INVALID, "n_q = %d outside 0 .. %d", s->n_q, ERPL_RW_MAX_Q);
  for (int k = 0; k < s->n_q; ++k)
    if (!(s->q[k] >= 0.0 && s->q[k] <= 1.0)) return erpl_fail(ERPL_ERR_INVALID, "q[%d] = %g outside [0, 1]", k, s->q[k]);
  if (!factors) return erpl_fail(ERPL_ERR_INVALID, "factors is NULL");
  if (!summary) return erpl_fail(ERPL_ERR_INVALID, "summary is NULL");
  if (!result) return erpl_fail(ERPL_ERR_INVALID, "result is NULL");
  if (n < 1 || n > kMostColumns) return erpl_fail(ERPL_ERR_INVALID, "n = %lld outside 1 .. 2^31 - 1", (long long)n);
  if (ld < n) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below n = %lld", (long long)ld, (long long)n);
  if (ld_s < n) return erpl_fail(ERPL_ERR_INVALID, "ld_s = %lld is below n = %lld", (long long)ld_s, (long long)n);
  return ERPL_OK;
}

int launch_passes(const RwArgs& a, const ErplRwLaw& law, hipStream_t st) {
  const int nb = grid_of(a.n);
  RwWork* w = a.work;
  hipError_t e = hipMemsetAsync(&w->hist[0][0][0], 0, sizeof(w->hist), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rw_logw, dim3(nb), dim3(kBlock), 0, st, a, law);
  hipLaunchKernelGGL(rw_finish_max, dim3(1), dim3(kBlock), 0, st, w, nb);
  hipLaunchKernelGGL(rw_weights, dim3(nb), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(rw_finish_weights, dim3(1), dim3(kBlock), 0, st, w, nb);
  hipLaunchKernelGGL(rw_rows<false>, dim3(nb, a.n_rows), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(rw_finish_rows<false>, dim3(a.n_rows), dim3(kBlock), 0, st, a, nb);
  hipLaunchKernelGGL(rw_rows<true>, dim3(nb, a.n_rows), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(rw_finish_rows<true>, dim3(a.n_rows), dim3(kBlock), 0, st, a, nb);
  if (a.n_q > 0)
    for (int shift = 56; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(rw_hist, dim3(nb, a.n_rows), dim3(kBlock), 0, st, a, shift);
      hipLaunchKernelGGL(rw_scan, dim3(a.n_rows), dim3(64 * kQ), 0, st, a, shift);
    }
  return (int)hipGetLastError();
}
}  // namespace

extern "C" {

int erpl_mc_reweight_defaults(erpl_rw_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  *spec = erpl_rw_spec{};
  spec->n_law = 1;
  spec->kind[0] = ERPL_DESIGN_NORMAL;
  for (int r = 0; r < ERPL_RW_MAX_LAW; ++r) { spec->mu[r] = 0.0; spec->s[r] = 1.0; spec->a[r] = 0.0; spec->b[r] = 1.0; }
  spec->n_rows = 3;
  spec->rows[0] = ERPL_SUM_APOGEE_ALT; spec->rows[1] = ERPL_SUM_RANGE; spec->rows[2] = ERPL_SUM_FLIGHT_TIME;
  const double q[5] = {0.05, 0.25, 0.5, 0.75, 0.95};
  spec->n_q = 5;
  for (int k = 0; k < 5; ++k) spec->q[k] = q[k];
  return ERPL_OK;
}

int erpl_mc_reweight(erpl_ctx* c, const erpl_rw_spec* spec, const double* factors, int64_t ld, const double* summary, int64_t ld_s,
                     const double* extra, const uint8_t* mask, int64_t n, erpl_reweight* result, double* logw, int64_t* weights,
                     void* stream) {
  ERPL_TRY(reweight_check(spec, factors, ld, summary, ld_s, extra, n, result));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->reweight_pin) HIP_TRY(hipHostMalloc((void**)&c->reweight_pin, sizeof(ErplRwRaw), hipHostMallocDefault));
  const ErplRwLayout lay = erpl_rw_layout(n, logw != nullptr, weights != nullptr, sizeof(RwWork));
  ERPL_TRY(c->reweight.grow(lay.need));
  char* base = c->reweight.buf;
  hipStream_t st = (hipStream_t)stream;
  RwArgs a = {};
  a.factors = factors; a.summary = summary; a.extra = extra; a.mask = mask;
  a.logw = logw ? logw : (double*)(base + lay.logw);
  a.weights = weights ? weights : (int64_t*)(base + lay.weights);
  a.work = (RwWork*)(base + lay.work);
  a.ld = ld; a.ld_s = ld_s; a.n = n;
  a.n_rows = spec->n_rows; a.n_q = spec->n_q; a.Q = erpl_rw_q(n);
  for (int j = 0; j < spec->n_rows; ++j) {
    a.rows[j] = spec->rows[j];
    a.n_thr[j] = spec->n_thresholds[j];
    for (int k = 0; k < spec->n_thresholds[j]; ++k) a.thr[j][k] = spec->threshold[j][k];
  }
  for (int k = 0; k < spec->n_q; ++k) a.q[k] = spec->q[k];
  KERNEL_TRY(launch_passes(a, erpl_rw_law_of(*spec), st));
  ErplRwRaw* raw = (ErplRwRaw*)c->reweight_pin;
  HIP_TRY(hipMemcpyAsync(raw, &a.work->raw, sizeof(ErplRwRaw), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  erpl_rw_result(*spec, *raw, n, result);
  return ERPL_OK;
}

int erpl_mc_reweight_host(const erpl_rw_spec* spec, const double* factors, int64_t ld, const double* summary, int64_t ld_s,
                          const double* extra, const uint8_t* mask, int64_t n, erpl_reweight* result, double* logw, int64_t* weights) {
  ERPL_TRY(reweight_check(spec, factors, ld, summary, ld_s, extra, n, result));
  erpl_rw_host(*spec, factors, ld, summary, ld_s, extra, mask, n, result, logw, weights);
  return ERPL_OK;
}

}  // extern "C"
