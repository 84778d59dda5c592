// erpl_corridor_w.hip — erpl_mc_corridor_bands_weighted of the C ABI (include/erpl_mc.h): every (channel, node) row of a
// time-resolved matrix described under the integer weights erpl_mc_reweight wrote.  The rule is erpl_bands_w.h, here for the
// device (the kernels below) and for the host (erpl_mc_corridor_bands_weighted_host).
//
//   bw_scan / bw_scan_finish  the first pass, over the weight row alone, on grid_of(m) workgroups: the largest admitted weight,
//                             the lowest column whose weight is not admitted, the non-zero mask bytes.  The host waits for it:
//                             a weight outside 0 .. 2^Q refuses the call before a row record is written, and K is settled.
//   bw_rows                   THE hot kernel, one workgroup per row and one launch for all rows, the shape of
//                             erpl_corridor_bands: a moments pass, a centred pass, then the eight digit passes of the radix
//                             selection of erpl_stat_device.h with W in the place of 1 (select_count on 64-bit bins, select_scan),
//                             its 64-bit histograms in LDS alone (16 KB), one target per quantile.  A row is read ten times by one
//                             workgroup, so every pass keeps kLoads columns per thread in flight, the weight next to the value.
//                             The eight passes are select_row of erpl_stat_device.h written out with a weight: the shared body
//                             measured a little slower here (profiles/select_refactor_ab.json) and no cause was found, so the
//                             kernel stays as it was.  A fix to the pass structure there has to be made here as well.
// Sums are accumulated per thread in index order (thread t: t, t + 256, ..) and folded in the fixed order of
// erpl_stat_device.h: the order depends on m alone.  Integer LDS atomics only.  Compiled with -ffp-contract=off: w * x,
// (x - mean)^2 and the products with w round once each, as the host twin rounds them.
#include "erpl_host.h"

#include "erpl_bands_w.h"
#include "erpl_stat_device.h"

namespace {
constexpr int kBlock = ERPL_ANA_BLOCK;           // 256: the folds of erpl_stat_device.h are written for it
constexpr int kMaxBlocks = ERPL_ANA_MAX_BLOCKS;
constexpr int kQ = ERPL_RW_MAX_Q, kT = ERPL_BANDS_W_MAX_THRESHOLDS, kC = ERPL_CORRIDOR_MAX_CHANNELS;
constexpr int kLoads = 4;                        // kBandLoads of erpl_corridor.hip

// the first pass's piece of the workspace: what it hands back and a slot per workgroup for every partial
struct BwScanWork {
  ErplBwScan out;
  double p_max[kMaxBlocks], p_bad[kMaxBlocks];
  u64 p_masked[kMaxBlocks];
};

struct BwArgs {
  const double* values;      // [n_channels][n_nodes][ld]
  const uint8_t* mask;       // [m] or NULL
  const int64_t* weights;    // [m]
  ErplBwRaw* out;            // [rows]
  int64_t m, ld;
  int32_t n_nodes, n_q;
  double scale;              // 2^-K
  double q[kQ];
  int32_t n_thr[kC];
  double thr[kC][kT];
};

// ---------------------------------------------------------------- the first pass

__global__ __launch_bounds__(kBlock) void bw_scan(const int64_t* __restrict__ wt, const uint8_t* __restrict__ mask, const int64_t m,
                                                  const int Q, BwScanWork* w) {
  const int64_t stride = (int64_t)gridDim.x * kBlock, most = (int64_t)1 << Q;
  double max_w = 0.0, bad = INFINITY;
  u64 masked = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
    const int64_t W = wt[i];
    if (W < 0 || W > most) {
      if ((double)i < bad) bad = (double)i;      // exact: i < 2^31
    } else {
      const double wd = (double)W;               // exact: W <= 2^52
      max_w = wd > max_w ? wd : max_w;
    }
    if (mask && mask[i] != 0) ++masked;
  }
  block_fold<Max, Min, Add>(max_w, bad, masked);
  if (threadIdx.x == 0) { w->p_max[blockIdx.x] = max_w; w->p_bad[blockIdx.x] = bad; w->p_masked[blockIdx.x] = masked; }
}

__global__ __launch_bounds__(kBlock) void bw_scan_finish(BwScanWork* w, const int nb) {
  double max_w = thread_partials<Max>(w->p_max, nb), bad = thread_partials<Min>(w->p_bad, nb);
  u64 masked = thread_partials<Add>(w->p_masked, nb);
  block_fold<Max, Min, Add>(max_w, bad, masked);
  if (threadIdx.x == 0) {
    w->out.n_masked = masked;
    w->out.max_w = (u64)max_w;
    w->out.first_bad = bad < (double)INFINITY ? (int64_t)bad : -1;
  }
}

// ---------------------------------------------------------------- the rows

// The columns i0, i0 + 256, .. of a row: value, weight and ok[k] = the column exists and its mask byte is 0.  A column past
// the row is 0.0 with weight 0, never read from memory.
__device__ __forceinline__ void bw_fetch(const double* __restrict__ x, const int64_t* __restrict__ wt, const uint8_t* __restrict__ mask,
                                         int64_t m, int64_t i0, double (&v)[kLoads], u64 (&W)[kLoads], bool (&ok)[kLoads]) {
  uint8_t byte[kLoads];
#pragma unroll
  for (int k = 0; k < kLoads; ++k) {
    const int64_t i = i0 + (int64_t)k * kBlock;
    ok[k] = i < m;
    v[k] = ok[k] ? x[i] : 0.0;
    W[k] = ok[k] ? (u64)wt[i] : 0ull;
    byte[k] = ok[k] && mask ? mask[i] : (uint8_t)0;
  }
#pragma unroll
  for (int k = 0; k < kLoads; ++k) ok[k] = ok[k] && byte[k] == 0;
}

__global__ __launch_bounds__(kBlock) void bw_rows(const BwArgs a) {
  __shared__ u64 s_hist[kQ][ERPL_ANA_BINS];      // 16 KB
  __shared__ u64 s_prefix[kQ], s_rank[kQ];       // per target
  __shared__ int s_leader[kQ];
  __shared__ u64 s_lead_prefix[kQ];              // per group
  __shared__ int s_lead[kQ];
  __shared__ int s_nlead;
  __shared__ double s_mean;
  __shared__ u64 s_sum_w;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = a.n_q;
  const int64_t m = a.m;
  const int c = (int)blockIdx.x / a.n_nodes;
  const double* __restrict__ x = a.values + (int64_t)blockIdx.x * a.ld;
  const int64_t* __restrict__ wt = a.weights;
  const uint8_t* __restrict__ mask = a.mask;
  const double scale = a.scale;
  ErplBwRaw& o = a.out[blockIdx.x];
  const int n_thr = a.n_thr[c];
  double thr[kT];
#pragma unroll
  for (int j = 0; j < kT; ++j) thr[j] = a.thr[c][j];

  // moments, first pass; the columns that are open but not members on the way.  The extremes go by key: -0.0 below +0.0.
  double sum_wx = 0.0, sum_w2 = 0.0, a2[kT];
  u64 kmin = ~0ull, kmax = 0ull, cnt = 0ull, nnf = 0ull, nz = 0ull, sum_w = 0ull, ex[kT];
#pragma unroll
  for (int j = 0; j < kT; ++j) { a2[j] = 0.0; ex[j] = 0ull; }
  for (int64_t i0 = tid; i0 < m; i0 += kLoads * kBlock) {
    double v[kLoads];
    u64 W[kLoads];
    bool ok[kLoads];
    bw_fetch(x, wt, mask, m, i0, v, W, ok);
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {           // (index order: i0, i0 + 256, ..)
      if (!ok[k]) continue;
      if (!finite_bits(v[k])) { ++nnf; continue; }
      if (W[k] == 0ull) { ++nz; continue; }
      const double wd = (double)(int64_t)W[k] * scale;   // exact: W <= 2^52 and a power of two
      const double w2 = wd * wd;
      const u64 key = key_of_signed(v[k]);
      ++cnt;
      sum_w += W[k];
      sum_wx += wd * v[k];
      sum_w2 += w2;
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
#pragma unroll
      for (int j = 0; j < kT; ++j)
        if (j < n_thr && v[k] > thr[j]) { ex[j] += W[k]; a2[j] += w2; }
    }
  }
  block_fold<Add, Add, Min, Max, Add, Add, Add, Add>(sum_wx, sum_w2, kmin, kmax, cnt, nnf, nz, sum_w);
  if (tid == 0) {
    o.count = cnt; o.n_non_finite = nnf; o.n_zero = nz; o.sum_w = sum_w;
    o.sum_wx = sum_wx; o.sum_w2 = sum_w2;
    o.vmin = cnt ? erpl_double_of(erpl_tally_bits_of_key(kmin)) : (double)INFINITY;
    o.vmax = cnt ? erpl_double_of(erpl_tally_bits_of_key(kmax)) : -(double)INFINITY;
    o.mean = sum_wx / ((double)sum_w * scale);   // NaN for an empty row; the host reports every double of such a row as NaN
    s_mean = o.mean; s_sum_w = sum_w;
  }
#pragma unroll
  for (int j = 0; j < kT; ++j) {
    if (j < n_thr) block_fold_again<Add, Add>(ex[j], a2[j]);   // (uniform over the workgroup)
    if (tid == 0) { o.exceed[j] = j < n_thr ? ex[j] : 0ull; o.a2[j] = j < n_thr ? a2[j] : 0.0; }
  }
  __syncthreads();
  const double mean = s_mean;
  const u64 S = s_sum_w;

  // second pass
  double m2 = 0.0, se2 = 0.0;
  for (int64_t i0 = tid; i0 < m; i0 += kLoads * kBlock) {
    double v[kLoads];
    u64 W[kLoads];
    bool ok[kLoads];
    bw_fetch(x, wt, mask, m, i0, v, W, ok);
#pragma unroll
    for (int k = 0; k < kLoads; ++k)
      if (ok[k] && finite_bits(v[k]) && W[k] != 0ull) {
        const double wd = (double)(int64_t)W[k] * scale, d = v[k] - mean;
        const double dd = d * d;
        m2 += wd * dd;
        se2 += (wd * wd) * dd;
      }
  }
  block_fold<Add, Add>(m2, se2);
  if (tid == 0) { o.m2 = m2; o.se2 = se2; }

  // selection: every target starts with no digit fixed, in one group
  if (tid < kQ) {
    s_prefix[tid] = 0ull;
    s_rank[tid] = S > 0ull && tid < nt ? erpl_rw_target(a.q[tid], S) - 1ull : 0ull;
  }
  if (S > 0ull && nt > 0) {   // (uniform over the workgroup)
    for (int shift = 56; shift >= 0; shift -= 8) {
      __syncthreads();   // the prefixes of the pass before are in place, its histograms have been read
      for (int k = tid; k < kQ * ERPL_ANA_BINS; k += kBlock) (&s_hist[0][0])[k] = 0ull;
      if (tid < nt) s_leader[tid] = select_leader(s_prefix, tid);
      __syncthreads();
      if (tid == 0) {
        int g = 0;
        for (int t = 0; t < nt; ++t)
          if (s_leader[t] == t) { s_lead[g] = t; s_lead_prefix[g] = s_prefix[t]; ++g; }
        s_nlead = g;
      }
      __syncthreads();
      const int nlead = s_nlead;
      // uniform over the wave (ballots): every lane makes every call, a lane past the row brings no key
      for (int64_t base = (int64_t)wave * 64; base < m; base += kLoads * kBlock) {
        double v[kLoads];
        u64 W[kLoads];
        bool ok[kLoads];
        bw_fetch(x, wt, mask, m, base + lane, v, W, ok);
#pragma unroll
        for (int k = 0; k < kLoads; ++k)
          select_count(s_hist, s_lead, s_lead_prefix, nlead, ok[k] && finite_bits(v[k]) && W[k] != 0ull, key_of_signed(v[k]), shift,
                       W[k]);
      }
      __syncthreads();
      // wave w scans for the targets w, w + kWaves, ..: the digit that holds the rank, the rank within that bin
      for (int t = wave; t < nt; t += kWaves) {
        int d = 0;
        u64 below = 0ull;
        if (select_scan(s_hist[s_leader[t]], s_rank[t], lane, &d, &below)) {   // exactly one lane
          s_prefix[t] |= (u64)d << shift;
          s_rank[t] -= below;
        }
      }
    }
    __syncthreads();
  } else {
    __syncthreads();
  }
  if (tid < kQ) o.key[tid] = tid < nt ? s_prefix[tid] : 0ull;
}

// the workspace: the first pass's piece, then a record per row
constexpr size_t kRowsAt = (sizeof(BwScanWork) + 255) & ~(size_t)255;

int bw_fail_weight(int64_t column, int Q) {
  return erpl_fail(ERPL_ERR_INVALID, "weights[%lld] is outside 0 .. 2^%d", (long long)column, Q);
}
}  // namespace

extern "C" {

int erpl_mc_corridor_bands_weighted_defaults(erpl_bands_w_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  memset(spec, 0, sizeof(*spec));
  const double q[5] = {0.05, 0.25, 0.5, 0.75, 0.95};   // erpl_mc_corridor_defaults
  spec->n_q = 5;
  for (int k = 0; k < 5; ++k) spec->q[k] = q[k];
  return ERPL_OK;
}

int erpl_mc_corridor_bands_weighted(erpl_ctx* c, const double* values, const uint8_t* mask, const int64_t* weights, int64_t m,
                                    int64_t ld, const erpl_bands_w_spec* spec, erpl_bands_w_row* rows, erpl_bands_w_result* result,
                                    void* stream) {
  ERPL_TRY(erpl_bw_check(spec, values, weights, rows, result, m, ld, erpl_fail));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int n_rows = spec->n_channels * spec->n_nodes;
  ERPL_TRY(c->bands_w.grow(kRowsAt + (size_t)n_rows * sizeof(ErplBwRaw)));
  BwScanWork* scan_work = (BwScanWork*)c->bands_w.buf;

  const int nb = grid_of(m), Q = erpl_rw_q(m);
  hipLaunchKernelGGL(bw_scan, dim3(nb), dim3(kBlock), 0, st, weights, mask, m, Q, scan_work);
  hipLaunchKernelGGL(bw_scan_finish, dim3(1), dim3(kBlock), 0, st, scan_work, nb);
  KERNEL_TRY((int)hipGetLastError());
  ErplBwScan scan;
  HIP_TRY(hipMemcpyAsync(&scan, &scan_work->out, sizeof(scan), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (scan.first_bad >= 0) return bw_fail_weight(scan.first_bad, Q);

  const int K = erpl_bw_bits(scan.max_w);
  BwArgs a;
  memset(&a, 0, sizeof(a));
  a.values = values; a.mask = mask; a.weights = weights; a.out = (ErplBwRaw*)(c->bands_w.buf + kRowsAt);
  a.m = m; a.ld = ld; a.n_nodes = spec->n_nodes; a.n_q = spec->n_q; a.scale = ldexp(1.0, -K);
  for (int k = 0; k < spec->n_q; ++k) a.q[k] = spec->q[k];
  for (int ch = 0; ch < spec->n_channels; ++ch) {
    a.n_thr[ch] = spec->n_thresholds[ch];
    for (int k = 0; k < spec->n_thresholds[ch]; ++k) a.thr[ch][k] = spec->threshold[ch][k];
  }
  hipLaunchKernelGGL(bw_rows, dim3((unsigned)n_rows), dim3(kBlock), 0, st, a);
  KERNEL_TRY((int)hipGetLastError());
  std::vector<ErplBwRaw> raw((size_t)n_rows);
  HIP_TRY(hipMemcpyAsync(raw.data(), a.out, (size_t)n_rows * sizeof(ErplBwRaw), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int r = 0; r < n_rows; ++r) erpl_bw_finish(*spec, r / spec->n_nodes, raw[(size_t)r], K, &rows[r]);
  memset(result, 0, sizeof(*result));
  result->m = m; result->n_masked = (int64_t)scan.n_masked; result->n_counted = m - (int64_t)scan.n_masked;
  result->max_w = (int64_t)scan.max_w; result->K = K; result->Q = Q;
  return ERPL_OK;
}

int erpl_mc_corridor_bands_weighted_host(const double* values, const uint8_t* mask, const int64_t* weights, int64_t m, int64_t ld,
                                         const erpl_bands_w_spec* spec, erpl_bands_w_row* rows, erpl_bands_w_result* result) {
  ERPL_TRY(erpl_bw_check(spec, values, weights, rows, result, m, ld, erpl_fail));
  const int64_t bad = erpl_bw_host(*spec, values, mask, weights, m, ld, rows, result);
  if (bad >= 0) return bw_fail_weight(bad, erpl_rw_q(m));
  return ERPL_OK;
}

}  // extern "C"
