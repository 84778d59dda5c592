// erpl_stat_device.h — what the statistics units (erpl_analysis.hip, erpl_distributions.hip, erpl_correlation.hip,
// erpl_bootstrap.hip, erpl_density.hip, erpl_corridor.hip, erpl_sobol.hip, erpl_dependence.hip, erpl_compare.hip,
// erpl_reweight.hip, erpl_density_w.hip, erpl_corridor_depth.hip, erpl_corridor_w.hip) share:
// the grid of their streaming passes, the order-preserving keys, the run of equal keys behind a mid-rank, THE fixed-order
// reduction and the steps of the radix selection.
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

// ---- the most-significant-digit radix selection of erpl_analysis.hip and erpl_corridor.hip: one 8-bit digit per pass, a
// histogram per group of targets that still share a key prefix.  The units differ in where the histograms live (64-bit
// global bins behind LDS tiles there, LDS alone here); what a pass decides is written once, below.

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
__device__ __forceinline__ void select_count(unsigned int (*hist)[ERPL_ANA_BINS], const int* lead, const u64* prefix, int nlead,
                                             bool use, u64 key, int shift) {
  // bits above the digit of this pass (none in the first pass: every key matches)
  const u64 above = shift >= 56 ? 0ull : (~0ull << (shift + 8));
  const unsigned int digit = (unsigned int)(key >> shift) & (ERPL_ANA_BINS - 1);
  for (int m = 0; m < nlead; ++m) {
    const bool hit = use && ((key ^ prefix[m]) & above) == 0ull;
    const u64 mask = __ballot(hit);
    if (mask == 0ull) continue;
    // heavily tied data puts a whole wave into one bin: one add of the lane count instead of 64 serialised ones
    const int lead_lane = __ffsll((long long)mask) - 1;
    const unsigned int d0 = (unsigned int)__shfl((int)digit, lead_lane);
    if (__ballot(hit && digit != d0) == 0ull) {
      if ((int)(threadIdx.x & 63) == lead_lane) atomicAdd(&hist[lead[m]][d0], (unsigned int)__popcll(mask));
    } else if (hit) {
      atomicAdd(&hist[lead[m]][digit], 1u);
    }
  }
}

// The weighted sibling (erpl_reweight.hip, erpl_density_w.hip, erpl_corridor_w.hip): the key counts w times, the bins are 64-bit.  A wave whose hits share one bin adds
// their weights up with a shuffle tree first (integer adds: the order does not matter) and makes one add of it.
__device__ __forceinline__ void select_count_weighted(u64 (*hist)[ERPL_ANA_BINS], const int* lead, const u64* prefix, int nlead,
                                                      bool use, u64 key, int shift, u64 w) {
  const u64 above = shift >= 56 ? 0ull : (~0ull << (shift + 8));
  const unsigned int digit = (unsigned int)(key >> shift) & (ERPL_ANA_BINS - 1);
  for (int m = 0; m < nlead; ++m) {
    const bool hit = use && ((key ^ prefix[m]) & above) == 0ull;
    const u64 mask = __ballot(hit);
    if (mask == 0ull) continue;
    const int lead_lane = __ffsll((long long)mask) - 1;
    const unsigned int d0 = (unsigned int)__shfl((int)digit, lead_lane);
    if (__ballot(hit && digit != d0) == 0ull) {
      u64 s = hit ? w : 0ull;
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
      if ((threadIdx.x & 63) == 0 && s) atomicAdd(&hist[lead[m]][d0], s);
    } else if (hit && w) {
      atomicAdd(&hist[lead[m]][digit], w);
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

}  // namespace
