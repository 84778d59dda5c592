// erpl_stat_device.h — what the statistics units (erpl_analysis.hip, erpl_distributions.hip, erpl_correlation.hip,
// erpl_bootstrap.hip, erpl_density.hip, erpl_corridor.hip, erpl_sobol.hip, erpl_dependence.hip, erpl_compare.hip,
// erpl_reweight.hip, erpl_density_w.hip, erpl_corridor_depth.hip, erpl_corridor_w.hip) share:
// the grid of their streaming passes, the order-preserving keys, the run of equal keys behind a mid-rank, THE fixed-order
// reduction and THE radix selection: its single steps (erpl_subset.hip and erpl_compare.hip select one target with them)
// and, around them, the passes of units that select many (erpl_analysis.hip, erpl_density_w.hip with bins in global
// memory; erpl_corridor.hip with bins in LDS alone; erpl_reweight.hip and erpl_corridor_w.hip keep copies of their own).
// Internal: never installed.
//
// The order is the contract: the last bit of every sum and the sign of a zero minimum depend on it, and "the same bits in
// every call" rests on it.  It is defined here and nowhere else:
//   1. a thread accumulates its own values in index order (the streaming loops of the units; thread_partials below);
//   2. a wave folds with a __shfl_down tree over the offsets 32, 16, .. 1: lane l takes lane l + off as the incoming value;
//   3. lane 0 of every wave parks its value in LDS;
//   4. thread 0 folds the waves 1, 2, .. onto its own (wave 0), in that order.  The result is valid in thread 0 only.
// The partials of the workgroups are folded the same way by one workgroup: thread t takes the partials t * kPer ..
// t * kPer + kPer - 1 in index order, then steps 2 - 4.  In every step the value a thread holds is the running one.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "erpl_tables.h"

namespace {

typedef unsigned long long u64;
constexpr int kWaves = ERPL_ANA_BLOCK / 64;
constexpr int kPer = ERPL_ANA_MAX_BLOCKS / ERPL_ANA_BLOCK;   // partials per thread of a finishing workgroup

// the grid of every streaming pass: a function of n alone (also on the device: erpl_density.hip sizes the passes over its
// dense population by the count the select left there)
__host__ __device__ inline int grid_of(int64_t n) {
  const int64_t want = (n + ERPL_ANA_BLOCK - 1) / ERPL_ANA_BLOCK;
  return (int)(want < ERPL_ANA_MAX_BLOCKS ? want : ERPL_ANA_MAX_BLOCKS);
}

__device__ __forceinline__ bool finite_bits(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

// Two order-preserving maps of a finite double onto an unsigned key.  They differ in the zeros alone:
//   key_of_signed   -0.0 sorts just below +0.0.  The selection of erpl_analysis.hip returns a value of the row, sign of a
//                   zero included (double_of_key in erpl_stats_api.hip inverts the map).
//   key_of_tied     -0.0 and +0.0 share one key.  The ranks of erpl_correlation.hip tie them, as scipy.stats.rankdata does.
__device__ __forceinline__ u64 key_of_signed(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
__device__ __forceinline__ u64 key_of_tied(double v) { return key_of_signed(v == 0.0 ? 0.0 : v); }

// The rank step of erpl_correlation.hip and erpl_dependence.hip: keys[0 .. count - 1] ascending, p < count.  The run of keys
// equal to keys[p] is [*first, *last]; both ends by galloping away from p, then bisection: O(log len) reads next to p.  The
// 1-based mid-rank of the run is *first + (len + 1) / 2, and 2 rank - 1 = *first + *last + 1.
__device__ __forceinline__ void run_of_key(const u64* __restrict__ keys, const int64_t p, const int64_t count, int64_t* first_out,
                                           int64_t* last_out) {
  const u64 k = keys[p];
  int64_t first = p, last = p;
  if (p > 0 && keys[p - 1] == k) {
    int64_t eq = p - 1, step = 1;   // keys[eq] == k
    while (eq - step >= 0 && keys[eq - step] == k) { eq -= step; step <<= 1; }
    int64_t ne = eq - step < 0 ? -1 : eq - step;   // keys[ne] != k, or before the row
    while (eq - ne > 1) {
      const int64_t m = ne + (eq - ne) / 2;
      if (keys[m] == k) eq = m; else ne = m;
    }
    first = eq;
  }
  if (p + 1 < count && keys[p + 1] == k) {
    int64_t eq = p + 1, step = 1;
    while (eq + step < count && keys[eq + step] == k) { eq += step; step <<= 1; }
    int64_t ne = eq + step < count ? eq + step : count;   // keys[ne] != k, or behind the population
    while (ne - eq > 1) {
      const int64_t m = eq + (ne - eq) / 2;
      if (keys[m] == k) eq = m; else ne = m;
    }
    last = eq;
  }
  *first_out = first;
  *last_out = last;
}

// ---- the operations of a fold: of(running, incoming), and the value that leaves every other one as it is
struct Add {
  template <class T> __device__ static T of(T run, T in) { return run + in; }
  template <class T> __device__ static T none() { return (T)0; }
};
struct Min {   // of two equal values (+0.0, -0.0) the running one stays
  template <class T> __device__ static T of(T run, T in) { return in < run ? in : run; }
  template <class T> __device__ static T none() {
    static_assert(std::is_floating_point<T>::value, "an extreme of floating-point values: the identity is an infinity");
    return (T)INFINITY;
  }
};
struct Max {
  template <class T> __device__ static T of(T run, T in) { return in > run ? in : run; }
  template <class T> __device__ static T none() {
    static_assert(std::is_floating_point<T>::value, "an extreme of floating-point values: the identity is an infinity");
    return (T)-INFINITY;
  }
};

// The folds take several values at once, each with its own operation: block_fold<Add, Min>(sum, mn).  The values are
// independent, so their shuffles interleave and one pair of barriers serves them all.  Every value is a double or a u64;
// LDS holds it as its 64 bits.
template <class T>
__device__ __forceinline__ u64 bits_of(T v) {
  static_assert(sizeof(T) == sizeof(u64), "a double or a u64");
  u64 b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}
template <class T>
__device__ __forceinline__ T from_bits(u64 b) {
  T v;
  __builtin_memcpy(&v, &b, sizeof(v));
  return v;
}

// step 2.  Valid in lane 0.
template <class... Op, class... T>
__device__ __forceinline__ void wave_fold(T&... v) {
  for (int off = 32; off > 0; off >>= 1) ((v = Op::of(v, __shfl_down(v, off))), ...);
}

// steps 2 - 4 over a workgroup of ERPL_ANA_BLOCK threads, all of which call it.  Valid in thread 0.  The LDS scratch
// belongs to the combination of operations and types.  AGAIN: a kernel that calls one combination a second time passes
// true from the second call on, and the scratch is guarded against the reads of the call before; a first call needs no
// guard and pays for none.
// Two unguarded calls of one combination in one kernel are a data race on s_wave: the second has to be block_fold_again.
template <bool AGAIN, class... Op, class... T>
__device__ __forceinline__ void block_fold_impl(T&... v) {
  static_assert(sizeof...(Op) == sizeof...(T), "one operation per value");
  __shared__ u64 s_wave[kWaves][sizeof...(T)];
  wave_fold<Op...>(v...);
  if (AGAIN) __syncthreads();   // s_wave may still be read from the call before
  if ((threadIdx.x & 63) == 0) {
    u64* slot = s_wave[threadIdx.x >> 6];
    ((*slot++ = bits_of(v)), ...);
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kWaves; ++w) {
      const u64* slot = s_wave[w];
      ((v = Op::of(v, from_bits<T>(*slot++))), ...);
    }
}
template <class... Op, class... T>
__device__ __forceinline__ void block_fold(T&... v) { block_fold_impl<false, Op...>(v...); }
template <class... Op, class... T>
__device__ __forceinline__ void block_fold_again(T&... v) { block_fold_impl<true, Op...>(v...); }

// step 1 of a finishing workgroup: what thread t makes of the partials t * kPer .. t * kPer + kPer - 1 among the first
// nb <= ERPL_ANA_MAX_BLOCKS of p[0], p[stride], ..  block_fold does the rest.
template <class Op, class T>
__device__ __forceinline__ T thread_partials(const T* p, int nb, int stride = 1) {
  T v = Op::template none<T>();
  for (int k = 0; k < kPer; ++k) {
    const int j = threadIdx.x * kPer + k;
    if (j < nb) v = Op::of(v, p[(size_t)j * stride]);
  }
  return v;
}

// K counters a wave holds uniformly (sums of ballot counts): thread k < K returns counter k added over the waves, every
// other thread 0.  Integer adds commute; the barrier inside also orders the LDS traffic of the caller's loop before what
// follows the call.
template <int K>
__device__ __forceinline__ u64 counters_fold(const u64 (&cnt)[K]) {
  __shared__ u64 s_cnt[kWaves][K];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_cnt[threadIdx.x >> 6][k] = cnt[k];
  }
  __syncthreads();
  u64 s = 0ull;
  if (threadIdx.x < K)
    for (int w = 0; w < kWaves; ++w) s += s_cnt[w][threadIdx.x];
  return s;
}

// ---- the most-significant-digit radix selection: all order statistics of a row together, one 8-bit digit per pass, a
// histogram per group of targets that still share a key prefix.  A key counts once (32-bit LDS bins) or with an integer
// weight (64-bit bins).  The single steps come first; erpl_subset.hip and erpl_compare.hip, which select one target,
// call them directly.  The passes around them are written here, in two forms:
//   global bins     the row is streamed by grid_of(n) workgroups, whose LDS histograms are flushed to 64-bit global bins;
//                   one kernel per digit (select_pass) and one between the digits (select_step), the state in an
//                   ErplSelect: erpl_analysis.hip, erpl_density_w.hip
//   LDS alone       one workgroup owns the row and runs the eight digits inside one kernel (select_row): erpl_corridor.hip
// The callers bring what differs: how a column yields (use, key, weight), and the rule that turns a quantile into a rank.
// Three copies of these passes remain outside, each around the shared steps: rw_hist / rw_scan of erpl_reweight.hip and the
// last third of bw_rows of erpl_corridor_w.hip, which measured slower with the shared bodies (profiles/
// select_refactor_ab.json), and the replicate kernel of erpl_bootstrap.hip, which selects on 32-bit positions.

// The rank of target t among the cnt > 0 counted values of a row: targets 2 i and 2 i + 1 are the two order statistics
// behind quantile q (np.percentile, linear): lo = floor(q (cnt - 1)) and min(lo + 1, cnt - 1).
__device__ __forceinline__ u64 select_rank(u64 cnt, double q, int t) {
  const double pos = q * (double)(cnt - 1ull);
  u64 lo = (u64)floor(pos);
  if (lo > cnt - 1ull) lo = cnt - 1ull;
  return (t & 1) ? (lo + 1ull < cnt ? lo + 1ull : cnt - 1ull) : lo;
}

// One key into the LDS histograms of a pass: hist[lead[m]] counts the digit at `shift` of the keys that match
// prefix[m] above it, m < nlead.  Every lane of the wave calls it (ballots); use = false: the lane brings no key.
// Count is the type of an LDS bin and decides what a key counts for:
//   unsigned int   once; w is not looked at
//   u64            w times (an integer weight)
// Heavily tied data puts a whole wave into one bin: then the wave makes one add instead of 64 serialised ones - of the
// lane count, by the leading lane, or of the weights added up with a shuffle tree (integer adds: the order does not
// matter), by lane 0.
template <class Count>
__device__ __forceinline__ void select_count(Count (*hist)[ERPL_ANA_BINS], const int* lead, const u64* prefix, int nlead, bool use,
                                             u64 key, int shift, Count w) {
  constexpr bool kOnce = std::is_same<Count, unsigned int>::value;
  static_assert(kOnce || std::is_same<Count, u64>::value, "32-bit bins count keys, 64-bit bins add weights");
  // bits above the digit of this pass (none in the first pass: every key matches)
  const u64 above = shift >= 56 ? 0ull : (~0ull << (shift + 8));
  const unsigned int digit = (unsigned int)(key >> shift) & (ERPL_ANA_BINS - 1);
  for (int m = 0; m < nlead; ++m) {
    const bool hit = use && ((key ^ prefix[m]) & above) == 0ull;
    const u64 mask = __ballot(hit);
    if (mask == 0ull) continue;
    const int lead_lane = __ffsll((long long)mask) - 1;
    const unsigned int d0 = (unsigned int)__shfl((int)digit, lead_lane);
    if (__ballot(hit && digit != d0) == 0ull) {
      if constexpr (kOnce) {
        if ((int)(threadIdx.x & 63) == lead_lane) atomicAdd(&hist[lead[m]][d0], (unsigned int)__popcll(mask));
      } else {
        u64 s = hit ? w : 0ull;
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&hist[lead[m]][d0], s);
      }
    } else if (hit && (kOnce || w)) {
      atomicAdd(&hist[lead[m]][digit], kOnce ? (Count)1 : w);
    }
  }
}

// A wave scans the ERPL_ANA_BINS counts h of a target's group for the bin that holds `rank`.  True in exactly one lane
// (in none if the histogram is empty): there *digit is the bin and *below the count of keys in the bins before it.
template <class Count>
__device__ __forceinline__ bool select_scan(const Count* h, u64 rank, int lane, int* digit, u64* below) {
  u64 c[4], s = 0ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) { c[k] = (u64)h[lane * 4 + k]; s += c[k]; }
  u64 incl = s;
  for (int off = 1; off < 64; off <<= 1) {
    const u64 up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  u64 before = incl - s;
  if (!(before <= rank && rank < incl)) return false;
  int d = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (rank >= before + c[k] && d == k) { before += c[k]; d = k + 1; }
  *digit = lane * 4 + d;
  *below = before;
  return true;
}

// the first target that shares target t's prefix: the one that keeps the histogram of the group
__device__ __forceinline__ int select_leader(const u64* prefix, int t) {
  int lead = t;
  for (int u = t - 1; u >= 0; --u) if (prefix[u] == prefix[t]) lead = u;
  return lead;
}

// the groups of a pass: the leaders among the nt targets and their prefixes, in target order.  One thread.
__device__ __forceinline__ int select_groups(const int* leader, const u64* prefix, int nt, int* lead, u64* lead_prefix) {
  int g = 0;
  for (int t = 0; t < nt; ++t)
    if (leader[t] == t) { lead[g] = t; lead_prefix[g] = prefix[t]; ++g; }
  return g;
}

template <int THREADS>
__device__ __forceinline__ void select_clear(u64* bins, int count) {
  for (int k = threadIdx.x; k < count; k += THREADS) bins[k] = 0ull;
}

// target t of a selection that begins: no digit fixed, in one group with every other target
template <int NT, class Key>
__device__ __forceinline__ void select_start(ErplSelect<NT>& sel, Key* key, int t, u64 rank) {
  sel.prefix[t] = 0ull; sel.rank[t] = rank; sel.leader[t] = 0;
  key[t] = 0ull;
}

// ---- global bins.  The body of a digit pass, for a workgroup of ERPL_ANA_BLOCK threads on a grid of gridDim.x of them
// over the n columns of a row: the digit at `shift` of the keys that match a target's prefix above it, per group of
// targets (only its leader keeps a histogram), in LDS and from there into bins[leader].  fetch(i, &key, &w), i < n, says
// whether column i counts and, if so, gives its key and (64-bit bins) its weight; key and w come in as 0.
template <class Count, int NT, class Fetch>
__device__ __forceinline__ void select_pass(const ErplSelect<NT>& sel, u64 (*bins)[ERPL_ANA_BINS], int nt, int64_t n, int shift,
                                            Fetch fetch) {
  __shared__ Count s_hist[NT][ERPL_ANA_BINS];   // 16 KB
  __shared__ u64 s_prefix[NT];
  __shared__ int s_lead[NT];
  __shared__ int s_nlead;
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int k = threadIdx.x; k < NT * ERPL_ANA_BINS; k += ERPL_ANA_BLOCK) (&s_hist[0][0])[k] = 0;
  if (threadIdx.x == 0) s_nlead = select_groups(sel.leader, sel.prefix, nt, s_lead, s_prefix);
  __syncthreads();
  const int nlead = s_nlead;
  const int64_t first = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + (threadIdx.x & ~63);
  for (int64_t base = first; base < n; base += stride) {   // uniform over the wave (ballots below)
    const int64_t i = base + (threadIdx.x & 63);
    bool use = false;
    u64 key = 0ull;
    Count w = 0;
    if (i < n) use = fetch(i, &key, &w);
    select_count(s_hist, s_lead, s_prefix, nlead, use, key, shift, w);
  }
  __syncthreads();
  for (int m = 0; m < nlead; ++m) {
    const int t = s_lead[m];
    for (int b = threadIdx.x; b < ERPL_ANA_BINS; b += ERPL_ANA_BLOCK) {
      const Count c = s_hist[t][b];
      if (c) atomicAdd(&bins[t][b], (u64)c);
    }
  }
}

// Between the passes, for ONE workgroup of 64 NT threads: wave t scans the histogram of target t's group, fixes the digit
// that holds its rank (key[t] follows the prefix) and reduces the rank to that bin; then the groups are formed again and
// the bins are cleared.
template <int NT, class Key>
__device__ __forceinline__ void select_step(ErplSelect<NT>& sel, u64 (*bins)[ERPL_ANA_BINS], Key* key, int nt, int shift) {
  __shared__ u64 s_prefix[NT];
  const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (t < nt) {
    const u64* h = bins[sel.leader[t]];
    const u64 rank = sel.rank[t];
    u64 prefix = sel.prefix[t], before = 0ull;
    int d = 0;
    if (lane == 0) s_prefix[t] = prefix;             // stays if no bin holds the rank: an empty row
    if (select_scan(h, rank, lane, &d, &before)) {   // exactly one lane
      prefix |= (u64)d << shift;
      sel.prefix[t] = prefix;
      sel.rank[t] = rank - before;
      key[t] = prefix;
      s_prefix[t] = prefix;
    }
  }
  __syncthreads();   // every histogram has been read, every prefix is known
  if (lane == 0 && t < nt) sel.leader[t] = select_leader(s_prefix, t);
  select_clear<64 * NT>(&bins[0][0], NT * ERPL_ANA_BINS);
}

// ---- LDS alone: one workgroup of ERPL_ANA_BLOCK threads per row of m columns, a key counting once.

// The columns i0, i0 + 256, .. of a row, LOADS loads per thread in flight: the value and ok[k] = the column exists and its
// mask byte is 0.  A value past the row is 0.0, never read from memory.
template <int LOADS>
__device__ __forceinline__ void band_fetch(const double* __restrict__ x, const uint8_t* __restrict__ mask, int64_t m, int64_t i0,
                                           double (&v)[LOADS], bool (&ok)[LOADS]) {
  uint8_t byte[LOADS];
#pragma unroll
  for (int k = 0; k < LOADS; ++k) {
    const int64_t i = i0 + (int64_t)k * ERPL_ANA_BLOCK;
    ok[k] = i < m;
    v[k] = ok[k] ? x[i] : 0.0;
    byte[k] = ok[k] && mask ? mask[i] : (uint8_t)0;
  }
#pragma unroll
  for (int k = 0; k < LOADS; ++k) ok[k] = ok[k] && byte[k] == 0;
}

// The whole selection of a row: nt <= NT targets, target t at rank_of(t) among the count > 0 finite unmasked values;
// count = 0 or nt = 0: no pass.  Every target starts with no digit fixed; then eight passes of {clear, leaders, groups,
// count, scan}.  key[t] = the key of target t, 0 for t >= nt and for an empty row.  Every thread calls it; the barriers
// inside also order what the caller put into LDS before the call.
template <int NT, int LOADS, class RankOf, class Key>
__device__ __forceinline__ void select_row(const double* __restrict__ x, const uint8_t* __restrict__ mask, int64_t m, int nt, u64 count,
                                           RankOf rank_of, Key* key) {
  __shared__ unsigned int s_hist[NT][ERPL_ANA_BINS];   // 16 KB
  __shared__ u64 s_prefix[NT], s_rank[NT];             // per target
  __shared__ int s_leader[NT];
  __shared__ u64 s_lead_prefix[NT];                    // per group
  __shared__ int s_lead[NT];
  __shared__ int s_nlead;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < NT) {
    s_prefix[tid] = 0ull;
    s_rank[tid] = count > 0ull && tid < nt ? rank_of(tid) : 0ull;
  }
  if (count > 0ull && nt > 0) {   // (uniform over the workgroup)
    for (int shift = 56; shift >= 0; shift -= 8) {
      __syncthreads();   // the prefixes of the pass before are in place, its histograms have been read
      for (int k = tid; k < NT * ERPL_ANA_BINS; k += ERPL_ANA_BLOCK) (&s_hist[0][0])[k] = 0u;
      if (tid < nt) s_leader[tid] = select_leader(s_prefix, tid);
      __syncthreads();
      if (tid == 0) s_nlead = select_groups(s_leader, s_prefix, nt, s_lead, s_lead_prefix);
      __syncthreads();
      const int nlead = s_nlead;
      // uniform over the wave (ballots): every lane makes every call, a lane past the row brings no key
      for (int64_t base = (int64_t)wave * 64; base < m; base += LOADS * ERPL_ANA_BLOCK) {
        double v[LOADS];
        bool ok[LOADS];
        band_fetch(x, mask, m, base + lane, v, ok);
#pragma unroll
        for (int k = 0; k < LOADS; ++k)
          select_count(s_hist, s_lead, s_lead_prefix, nlead, ok[k] && finite_bits(v[k]), key_of_signed(v[k]), shift, 1u);
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
  }
  __syncthreads();
  if (tid < NT) key[tid] = tid < nt ? s_prefix[tid] : 0ull;
}

}  // namespace
