// erpl_corridor.hip — the device passes of the trajectory corridor: erpl_mc_corridor_resample brings the ragged captured
// trajectories of a run onto one time grid, erpl_mc_corridor_bands describes every (channel, node) row of the resampled
// matrix.  No reference counterpart: plot_trajectory_cloud draws the first 50 trajectories as lines from Python lists.
//
//   resample   one workgroup per trajectory.  Pass 1 finds the usable prefix u.  "The first record with a non-finite
//              entry" is the record of the first non-finite element of the trajectory's records read as ONE flat array of
//              len * 15 doubles, so the pass streams that array with 16-byte loads, consecutive lanes at consecutive
//              addresses, four loads in flight per thread - every cache line is requested once, nothing goes through LDS
//              (47 % of the HBM rate against 23 % for a column-wise pass).  Then thread t takes
//              the nodes t, t + 256, ..: a bisection on the time column and the two records around the node (L2 hits: pass 1
//              has just streamed them).  The stores are 8 bytes, ld apart.
//   bands      one workgroup per row, one launch for all rows: moments in two passes, then the radix selection of
//              erpl_stat_device.h with its histograms in LDS alone - a row is read ten times by one workgroup.
// Sums are accumulated per thread in index order (thread t: t, t + 256, ..) and folded in the fixed order of
// erpl_stat_device.h: the order depends on m alone.  Integer LDS atomics only.  Compiled with -ffp-contract=off: the
// interpolation and (x - mean)^2 are rounded as NumPy rounds them.
#include "erpl_stat_device.h"

namespace {

// ---- resample

// channel ch of one record (absolute time + 14 state entries; x y z at 1..3, vx vy vz at 4..6)
__device__ __forceinline__ double channel_of(const double* __restrict__ rec, int ch) {
  if (ch == ERPL_CH_DOWNRANGE) {
    const double x = rec[1], y = rec[2];
    return sqrt(x * x + y * y);
  }
  if (ch == ERPL_CH_SPEED) {
    const double vx = rec[4], vy = rec[5], vz = rec[6];
    return sqrt((vx * vx + vy * vy) + vz * vz);
  }
  return rec[ch < ERPL_CH_DOWNRANGE ? 1 + ch : ch];   // X Y Z -> 1 2 3, VX VY VZ (4 5 6) -> 4 5 6
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corridor_resample(const ErplCorridorResampleArgs a) {
  __shared__ u64 s_first_bad;
  const int tid = threadIdx.x;
  const int64_t j = blockIdx.x;
  if (j >= a.n_traj) return;
  int64_t len = a.traj_len[j];
  len = (len < 0) ? 0 : ((len > a.traj_cap) ? a.traj_cap : len);   // never past the trajectory's own slots
  const double* __restrict__ recs = a.traj + j * a.traj_cap * ERPL_TRAJ_DIM;

  // pass 1: the first non-finite element of the flat array [0, total).  One element in front if the array starts 8 bytes
  // off a 16-byte boundary, then pairs, then one element behind if one is left.  A thread's indices increase: it keeps the
  // lowest hit of its first group of loads with one and stops there.
  const u64 none = ~0ull;
  const int64_t total = len * ERPL_TRAJ_DIM;
  const int64_t head = (((uintptr_t)recs & 15) != 0 && total > 0) ? 1 : 0;
  const int64_t pairs = (total - head) / 2;
  u64 bad = none;
  if (tid == 0 && head && !finite_bits(recs[0])) bad = 0ull;
  const double2* __restrict__ p2 = (const double2*)(recs + head);
  int64_t i = tid;
  // four loads in flight per thread before the first of them is looked at
  for (; bad == none && i + 3 * ERPL_ANA_BLOCK < pairs; i += 4 * ERPL_ANA_BLOCK) {
    double2 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p2[i + k * ERPL_ANA_BLOCK];
#pragma unroll
    for (int k = 3; k >= 0; --k) {   // (downwards: the lowest index is assigned last)
      if (!finite_bits(v[k].y)) bad = (u64)(head + 2 * (i + k * ERPL_ANA_BLOCK) + 1);
      if (!finite_bits(v[k].x)) bad = (u64)(head + 2 * (i + k * ERPL_ANA_BLOCK));
    }
  }
  for (; bad == none && i < pairs; i += ERPL_ANA_BLOCK) {
    const double2 v = p2[i];
    if (!finite_bits(v.y)) bad = (u64)(head + 2 * i + 1);
    if (!finite_bits(v.x)) bad = (u64)(head + 2 * i);
  }
  const int64_t last = head + 2 * pairs;   // == total - 1 if one element is left, else total
  if (tid == ERPL_ANA_BLOCK - 1 && last < total && !finite_bits(recs[last]) && (u64)last < bad) bad = (u64)last;
  block_fold<Min>(bad);
  if (tid == 0) s_first_bad = bad;
  __syncthreads();
  const u64 first_bad = s_first_bad;
  const int64_t u = first_bad == none ? len : (int64_t)(first_bad / ERPL_TRAJ_DIM);

  const bool hold = a.hold != 0 && u == len;   // a trajectory cut off by a non-finite record never holds
  const double t_first = u > 0 ? recs[0] : 0.0;
  const double t_end = u > 0 ? recs[(u - 1) * ERPL_TRAJ_DIM] - t_first : 0.0;
  double* __restrict__ col = a.values + a.col0 + j;
  for (int k = tid; k < a.n_nodes; k += ERPL_ANA_BLOCK) {
    const double tk = a.t0 + (double)k * a.dt;
    int64_t r = -1;      // the record at or before the node; -1: the node has no value
    bool exact = true;   // the value is ch(r) itself
    if (u > 0 && !(tk < 0.0)) {
      if (tk > t_end) {
        if (hold) r = u - 1;
      } else {
        // the largest r < u with ts(r) <= tk: ts(0) = 0 <= tk; whatever the stamps hold, lo and hi stay in [0, u]
        int64_t lo = 0, hi = u;
        while (hi - lo > 1) {
          const int64_t mid = lo + (hi - lo) / 2;
          if (recs[mid * ERPL_TRAJ_DIM] - t_first <= tk) lo = mid; else hi = mid;
        }
        r = lo;
        exact = r == u - 1;
      }
    }
    const double* __restrict__ r0 = recs + (r < 0 ? 0 : r) * ERPL_TRAJ_DIM;
    double w = 0.0;
    if (!exact) {
      const double ts0 = r0[0] - t_first, ts1 = r0[ERPL_TRAJ_DIM] - t_first;
      w = (tk - ts0) / (ts1 - ts0);
    }
    for (int c = 0; c < a.n_channels; ++c) {
      double v = (double)NAN;
      if (r >= 0) {
        const int ch = a.channels[c];
        v = channel_of(r0, ch);
        if (!exact) v = v + (channel_of(r0 + ERPL_TRAJ_DIM, ch) - v) * w;
      }
      col[((int64_t)c * a.n_nodes + k) * a.ld] = v;
    }
  }
}

// ---- bands: row blockIdx.x of the matrix through the moments and the selection of a described row

// One workgroup reads a whole row and only 768 of them exist with the default spec, so every pass keeps kBandLoads loads
// per thread in flight (band_fetch of erpl_stat_device.h).
constexpr int kBandLoads = 4;

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corridor_bands(const ErplCorridorBandsArgs a) {
  __shared__ double s_mean;
  __shared__ u64 s_cnt;
  const int tid = threadIdx.x;
  const int64_t m = a.m;
  const double* __restrict__ x = a.values + (int64_t)blockIdx.x * a.ld;
  const uint8_t* __restrict__ mask = a.mask;
  ErplAnaRow& o = a.out[blockIdx.x];

  // moments, first pass; the columns that count at all on the way
  double sum = 0.0, mn = INFINITY, mx = -INFINITY;
  u64 cnt = 0ull, open = 0ull;
  for (int64_t i0 = tid; i0 < m; i0 += kBandLoads * ERPL_ANA_BLOCK) {
    double v[kBandLoads];
    bool ok[kBandLoads];
    band_fetch(x, mask, m, i0, v, ok);
#pragma unroll
    for (int k = 0; k < kBandLoads; ++k) {   // (index order: i0, i0 + 256, ..)
      if (!ok[k]) continue;
      ++open;
      if (finite_bits(v[k])) {
        sum += v[k];
        ++cnt;
        mn = v[k] < mn ? v[k] : mn;
        mx = v[k] > mx ? v[k] : mx;
      }
    }
  }
  block_fold<Add, Add, Add, Min, Max>(sum, cnt, open, mn, mx);
  if (tid == 0) {
    o.count = cnt; o.sum = sum; o.vmin = mn; o.vmax = mx;
    o.mean = sum / (double)cnt;   // NaN for an empty row; the host reports every double of such a row as NaN
    s_mean = o.mean; s_cnt = cnt;
    if (blockIdx.x == 0) {        // the record behind the rows
      ErplAnaRow& e = a.out[a.rows];
      e.count = open; e.sum = e.mean = e.m2 = e.vmin = e.vmax = 0.0;
      for (int t = 0; t < ERPL_ANA_TARGETS; ++t) e.key[t] = 0ull;
    }
  }
  __syncthreads();
  const double mean = s_mean;
  const u64 count = s_cnt;

  // second pass
  double m2 = 0.0;
  for (int64_t i0 = tid; i0 < m; i0 += kBandLoads * ERPL_ANA_BLOCK) {
    double v[kBandLoads];
    bool ok[kBandLoads];
    band_fetch(x, mask, m, i0, v, ok);
#pragma unroll
    for (int k = 0; k < kBandLoads; ++k)
      if (ok[k] && finite_bits(v[k])) {
        const double d = v[k] - mean;
        m2 += d * d;
      }
  }
  block_fold<Add>(m2);
  if (tid == 0) o.m2 = m2;

  // the selection: the two order statistics behind every quantile, among the finite unmasked values
  select_row<ERPL_ANA_TARGETS, kBandLoads>(x, mask, m, 2 * a.n_q, count,
                                           [&](int t) { return select_rank(count, a.q[t >> 1], t); }, o.key);
}

}  // namespace

int erpl_launch_corridor_resample(const ErplCorridorResampleArgs& a, void* stream) {
  hipLaunchKernelGGL(erpl_corridor_resample, dim3((unsigned)a.n_traj), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int erpl_launch_corridor_bands(const ErplCorridorBandsArgs& a, void* stream) {
  hipLaunchKernelGGL(erpl_corridor_bands, dim3((unsigned)a.rows), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
