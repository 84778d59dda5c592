// erpl_corridor_depth.hip — the device passes of erpl_mc_corridor_depth: the modified band depth and the modified epigraph index
// of every column of a time-resolved matrix, and the functional boxplot on top of them.  The definitions are the header
// comment of include/erpl_mc.h; the integer rules and the buffer layout are erpl_depth.h.
//
//   ranks       the hot pass, per channel: (a, b) = the members of the row's population strictly below / above every element,
//               as a pair of uint32 per element.  Two paths that give the same integers:
//                 LDS     one workgroup per row: the row's keys (columns outside the population: the largest key) staged in
//                         LDS over the next power of two, a bitonic network over the keys alone, then every thread finds the
//                         run of its own key in the sorted row - a bisection for its lower bound, run_of_key for its end.
//                         The allocation is sized by m: small rows put several workgroups on a CU, a row of 16 384 columns
//                         takes 128 KB of the CU's 160 KB.
//                 global  the keys of a group of rows through rocPRIM's segmented radix sort (a row longer than
//                         ERPL_DEPTH_SEG_MAX: one device-wide sort of its own), then the same two searches in global memory
//   accumulate  a thread per column, the nodes in ascending order, coalesced reads of the pair matrix
//   select      per channel: the depths as keys through rocPRIM's radix sort; threshold, n_central and depth_max are read off
//               the sorted row, the median is the lowest column that holds the largest key
//   envelope    a workgroup per row: population, central members, their envelope and its fences
//   outliers    a thread per column: the nodes at which it leaves the fences, the central flag
//   whiskers    a workgroup per row: the envelope of the defined columns that never leave the fences
// Every floating-point sum is one thread's, in node order; the extremes fold in the fixed order of erpl_stat_device.h; the one
// atomic is an integer count.  Compiled with -ffp-contract=off: the terms, the sums and the fences round once per operation.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "erpl_depth.h"
#include "erpl_stat_device.h"

namespace {

// the key of column i of row x: the largest key outside the population (no finite double maps to it)
__device__ __forceinline__ u64 depth_key(const double* __restrict__ x, const uint8_t* __restrict__ mask, int64_t i) {
  if (mask && mask[i] != 0) return ~0ull;
  const double v = x[i];
  return finite_bits(v) ? key_of_tied(v) : ~0ull;
}

// the first position of keys[0 .. count - 1] (ascending) that holds a key >= k; count if none does
__device__ __forceinline__ int64_t lower_bound(const u64* keys, int64_t count, u64 k) {
  int64_t lo = 0, hi = count;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// (a, b) of a member with key k in the sorted population keys[0 .. n - 1]
__device__ __forceinline__ uint2 pair_of(const u64* keys, int64_t n, u64 k) {
  const int64_t a = lower_bound(keys, n, k);
  int64_t first, last;
  run_of_key(keys, a, n, &first, &last);
  return make_uint2((uint32_t)a, (uint32_t)(n - 1 - last));
}

// the inverse of key_of_signed
__device__ __forceinline__ double double_of_key(u64 k) {
  return from_bits<double>(k ^ ((k >> 63) ? (1ull << 63) : ~0ull));
}

// ---- ranks, LDS path: row blockIdx.x of the channel, nkeys = erpl_depth_lds_keys(m) keys in dynamic LDS
__global__ __launch_bounds__(ERPL_DEPTH_LDS_MAX_THREADS) void erpl_depth_rank_lds(const double* __restrict__ values, const int64_t ld,
                                                                                  const uint8_t* __restrict__ mask, const int m,
                                                                                  const int nkeys, uint2* __restrict__ pair,
                                                                                  int32_t* __restrict__ rown) {
  extern __shared__ u64 s_keys[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* __restrict__ x = values + (int64_t)blockIdx.x * ld;
  for (int i = tid; i < nkeys; i += nt) s_keys[i] = i < m ? depth_key(x, mask, i) : ~0ull;
  __syncthreads();
  // the bitonic network: thread i of a step holds the pair (lo, lo + j) of its compare-exchange
  for (int k = 2; k <= nkeys; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < nkeys / 2; i += nt) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int hi = lo + j;
        const bool up = (lo & k) == 0;
        const u64 p = s_keys[lo], q = s_keys[hi];
        if ((p > q) == up) { s_keys[lo] = q; s_keys[hi] = p; }
      }
      __syncthreads();
    }
  const int64_t n = lower_bound(s_keys, nkeys, ~0ull);   // uniform: every thread reads the same words
  if (tid == 0) rown[blockIdx.x] = (int32_t)n;
  uint2* __restrict__ out = pair + (int64_t)blockIdx.x * m;
  for (int i = tid; i < m; i += nt) {
    const u64 k = depth_key(x, mask, i);
    out[i] = k == ~0ull ? make_uint2(ERPL_DEPTH_NONE, ERPL_DEPTH_NONE) : pair_of(s_keys, n, k);
  }
}

// ---- ranks, global path: rows row0 + blockIdx.y of the channel; keys[blockIdx.y][m]
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_keys(const double* __restrict__ values, const int64_t ld,
                                                                  const uint8_t* __restrict__ mask, const int64_t m, const int row0,
                                                                  u64* __restrict__ keys) {
  const double* __restrict__ x = values + (int64_t)(row0 + blockIdx.y) * ld;
  u64* __restrict__ out = keys + (int64_t)blockIdx.y * m;
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < m; i += stride) out[i] = depth_key(x, mask, i);
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_offsets(uint32_t* __restrict__ offs, const int64_t m, const int rows) {
  const int i = blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x;
  if (i <= rows) offs[i] = (uint32_t)((int64_t)i * m);
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_lookup(const double* __restrict__ values, const int64_t ld,
                                                                    const uint8_t* __restrict__ mask, const int64_t m, const int row0,
                                                                    const u64* __restrict__ sorted, uint2* __restrict__ pair,
                                                                    int32_t* __restrict__ rown) {
  __shared__ int64_t s_n;
  const int row = row0 + blockIdx.y;
  const double* __restrict__ x = values + (int64_t)row * ld;
  const u64* __restrict__ keys = sorted + (int64_t)blockIdx.y * m;
  if (threadIdx.x == 0) {
    s_n = lower_bound(keys, m, ~0ull);
    if (blockIdx.x == 0) rown[row] = (int32_t)s_n;
  }
  __syncthreads();
  const int64_t n = s_n;
  uint2* __restrict__ out = pair + (int64_t)row * m;
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < m; i += stride) {
    const u64 k = depth_key(x, mask, i);
    out[i] = k == ~0ull ? make_uint2(ERPL_DEPTH_NONE, ERPL_DEPTH_NONE) : pair_of(keys, n, k);
  }
}

// ---- accumulate: column j of the channel over its nodes in ascending order
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_accumulate(const uint2* __restrict__ pair, const int32_t* __restrict__ rown,
                                                                        const int64_t m, const int T, double* __restrict__ depth,
                                                                        double* __restrict__ mei, int32_t* __restrict__ nodes) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t j = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; j < m; j += stride) {
    double sd = 0.0, sm = 0.0;
    int32_t cnt = 0;
    for (int k = 0; k < T; ++k) {
      const int64_t n = rown[k];
      if (n < 2) continue;
      const uint2 p = pair[(int64_t)k * m + j];
      if (p.x == ERPL_DEPTH_NONE) continue;
      sd += erpl_depth_term(n, p.x, p.y);
      sm += erpl_depth_mei_term(n, p.x);
      ++cnt;
    }
    depth[j] = cnt ? sd / (double)cnt : (double)NAN;
    mei[j] = cnt ? sm / (double)cnt : (double)NAN;
    nodes[j] = cnt;
  }
}

// ---- select: the depths of a channel as keys (an undefined column: the largest key), and what the sorted keys say
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_dkeys(const double* __restrict__ depth, const int32_t* __restrict__ nodes,
                                                                   const int64_t m, u64* __restrict__ keys) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t j = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; j < m; j += stride)
    keys[j] = nodes[j] > 0 ? key_of_signed(depth[j]) : ~0ull;
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_select(const double* __restrict__ depth, const int32_t* __restrict__ nodes,
                                                                    const int64_t m, const u64* __restrict__ sorted, const double central,
                                                                    ErplDepthChan* __restrict__ chan) {
  const int64_t n_defined = lower_bound(sorted, m, ~0ull);   // uniform
  if (n_defined == 0) {
    if (threadIdx.x == 0) {
      chan->n_defined = chan->n_central = 0; chan->n_outliers = 0ull; chan->median = -1;
      chan->threshold = chan->depth_max = (double)NAN;
      chan->spare[0] = chan->spare[1] = 0;
    }
    return;
  }
  const int64_t h = erpl_depth_h(central, n_defined);
  const u64 thr = sorted[n_defined - h], top = sorted[n_defined - 1];
  u64 first = ~0ull;   // the lowest column that holds the largest depth
  for (int64_t j = threadIdx.x; j < m; j += ERPL_ANA_BLOCK)
    if (first == ~0ull && nodes[j] > 0 && key_of_signed(depth[j]) == top) first = (u64)j;
  block_fold<Min>(first);
  if (threadIdx.x == 0) {
    chan->n_defined = n_defined;
    chan->n_central = n_defined - lower_bound(sorted, n_defined, thr);
    chan->n_outliers = 0ull;
    chan->median = (int64_t)first;
    chan->threshold = double_of_key(thr);
    chan->depth_max = double_of_key(top);
    chan->spare[0] = chan->spare[1] = 0;
  }
}

// ---- envelope: row blockIdx.x = c * T + k of the matrix
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_envelope(const ErplDepthArgs a) {
  const int c = blockIdx.x / a.n_nodes;
  const int64_t m = a.m;
  const double* __restrict__ x = a.values + (int64_t)blockIdx.x * a.ld;
  const double* __restrict__ depth = a.depth + (int64_t)c * m;
  const uint8_t* __restrict__ mask = a.mask;
  const double thr = a.chan[c].threshold;   // NaN without a defined column: nothing is central
  u64 n = 0ull, ncen = 0ull, masked = 0ull;
  double lo = INFINITY, hi = -INFINITY;
  for (int64_t j = threadIdx.x; j < m; j += ERPL_ANA_BLOCK) {
    if (mask && mask[j] != 0) { ++masked; continue; }
    const double v = x[j];
    if (!finite_bits(v)) continue;
    ++n;
    if (depth[j] >= thr) {
      ++ncen;
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
  }
  block_fold<Add, Add, Add, Min, Max>(n, ncen, masked, lo, hi);
  if (threadIdx.x == 0) {
    erpl_depth_row& o = a.rows[blockIdx.x];
    const double nan = (double)NAN;
    o.count = (int64_t)n;
    o.n_central_here = (int64_t)ncen;
    o.central_lo = ncen ? lo : nan;
    o.central_hi = ncen ? hi : nan;
    o.fence_lo = o.fence_hi = nan;
    if (ncen) erpl_depth_fences(lo, hi, a.factor, &o.fence_lo, &o.fence_hi);
    o.whisker_lo = o.whisker_hi = nan;
    if (blockIdx.x == 0) a.count[0] = masked;
  }
}

// ---- outliers: column j of channel blockIdx.y over its nodes
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_outliers(const ErplDepthArgs a) {
  const int c = blockIdx.y, T = a.n_nodes;
  const int64_t m = a.m, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const erpl_depth_row* __restrict__ rows = a.rows + (int64_t)c * T;
  const double* __restrict__ x = a.values + (int64_t)c * T * a.ld;
  const double thr = a.chan[c].threshold;
  // (uniform over the wave: the ballot below)
  for (int64_t base = (int64_t)blockIdx.x * ERPL_ANA_BLOCK; base < m; base += stride) {
    const int64_t j = base + threadIdx.x;
    bool flagged = false;
    if (j < m) {
      int32_t n_out = 0, first = -1;
      if (!(a.mask && a.mask[j] != 0))
        for (int k = 0; k < T; ++k) {
          const double flo = rows[k].fence_lo, fhi = rows[k].fence_hi;
          if (!(finite_bits(flo) && finite_bits(fhi))) continue;
          const double v = x[(int64_t)k * a.ld + j];
          if (finite_bits(v) && (v < flo || v > fhi)) {
            if (n_out == 0) first = k;
            ++n_out;
          }
        }
      const int64_t at = (int64_t)c * m + j;
      const bool defined = a.nodes[at] > 0;
      a.n_out[at] = n_out;
      a.first_out[at] = first;
      a.central_flag[at] = (defined && a.depth[at] >= thr) ? 1 : 0;
      flagged = defined && n_out > 0;
    }
    const u64 hit = __ballot(flagged);
    if ((threadIdx.x & 63) == 0 && hit) atomicAdd(&a.chan[c].n_outliers, (u64)__popcll(hit));
  }
}

// ---- whiskers: row blockIdx.x = c * T + k
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_depth_whiskers(const ErplDepthArgs a) {
  const int c = blockIdx.x / a.n_nodes;
  const int64_t m = a.m;
  const double* __restrict__ x = a.values + (int64_t)blockIdx.x * a.ld;
  const int32_t* __restrict__ nodes = a.nodes + (int64_t)c * m;
  const int32_t* __restrict__ n_out = a.n_out + (int64_t)c * m;
  const uint8_t* __restrict__ mask = a.mask;
  u64 cnt = 0ull;
  double lo = INFINITY, hi = -INFINITY;
  for (int64_t j = threadIdx.x; j < m; j += ERPL_ANA_BLOCK) {
    if (mask && mask[j] != 0) continue;
    const double v = x[j];
    if (!finite_bits(v) || nodes[j] <= 0 || n_out[j] != 0) continue;
    ++cnt;
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  block_fold<Add, Min, Max>(cnt, lo, hi);
  if (threadIdx.x == 0 && cnt) {
    a.rows[blockIdx.x].whisker_lo = lo;
    a.rows[blockIdx.x].whisker_hi = hi;
  }
}

}  // namespace

int erpl_depth_temp_bytes(int64_t m, int group, size_t* bytes) {
  u64* none = nullptr;
  size_t one = 0, seg = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, one, none, none, (size_t)m, 0, 64, (hipStream_t)0);
  if (e != hipSuccess) return (int)e;
  if (group > 0 && m <= ERPL_DEPTH_SEG_MAX) {
    uint32_t* offs = nullptr;
    e = rocprim::segmented_radix_sort_keys(nullptr, seg, none, none, (unsigned)((int64_t)group * m), (unsigned)group, offs, offs + 1, 0,
                                           64, (hipStream_t)0);
    if (e != hipSuccess) return (int)e;
  }
  *bytes = one > seg ? one : seg;
  return 0;
}

int erpl_launch_depth(const ErplDepthArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t m = a.m;
  const int T = a.n_nodes, C = a.n_channels, nb = grid_of(m);
  const dim3 blk(ERPL_ANA_BLOCK);
  hipError_t e;
  size_t temp_bytes = a.temp_bytes;
  if (a.lds) {
    // more than 64 KB of dynamic LDS has to be allowed first
    e = hipFuncSetAttribute((const void*)erpl_depth_rank_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                            ERPL_DEPTH_LDS_MAX * (int)sizeof(u64));
    if (e != hipSuccess) return (int)e;
  } else if (m <= ERPL_DEPTH_SEG_MAX) {
    hipLaunchKernelGGL(erpl_depth_offsets, dim3((unsigned)(a.group / ERPL_ANA_BLOCK + 1)), blk, 0, st, a.offs, m, a.group);
  }
  u64* keys_in = a.keys;
  for (int c = 0; c < C; ++c) {
    const double* x = a.values + (int64_t)c * T * a.ld;
    double* depth = a.depth + (int64_t)c * m;
    double* mei = a.mei + (int64_t)c * m;
    int32_t* nodes = a.nodes + (int64_t)c * m;
    uint2* pair = (uint2*)a.pair;
    if (a.lds) {
      const int nkeys = erpl_depth_lds_keys(m);
      hipLaunchKernelGGL(erpl_depth_rank_lds, dim3((unsigned)T), dim3((unsigned)erpl_depth_lds_threads(m)), (size_t)nkeys * sizeof(u64), st, x,
                         a.ld, a.mask, (int)m, nkeys, pair, a.rown);
    } else {
      u64* keys_out = a.keys + (int64_t)a.group * m;
      for (int row0 = 0; row0 < T; row0 += a.group) {
        const int g = T - row0 < a.group ? T - row0 : a.group;
        hipLaunchKernelGGL(erpl_depth_keys, dim3((unsigned)nb, (unsigned)g), blk, 0, st, x, a.ld, a.mask, m, row0, keys_in);
        if (m <= ERPL_DEPTH_SEG_MAX) {
          e = rocprim::segmented_radix_sort_keys(a.temp, temp_bytes, keys_in, keys_out, (unsigned)((int64_t)g * m), (unsigned)g, a.offs,
                                                 a.offs + 1, 0, 64, st);
          if (e != hipSuccess) return (int)e;
        } else {
          for (int r = 0; r < g; ++r) {
            e = rocprim::radix_sort_keys(a.temp, temp_bytes, keys_in + (int64_t)r * m, keys_out + (int64_t)r * m, (size_t)m, 0, 64, st);
            if (e != hipSuccess) return (int)e;
          }
        }
        hipLaunchKernelGGL(erpl_depth_lookup, dim3((unsigned)nb, (unsigned)g), blk, 0, st, x, a.ld, a.mask, m, row0, (const u64*)keys_out,
                           pair, a.rown);
      }
    }
    hipLaunchKernelGGL(erpl_depth_accumulate, dim3((unsigned)nb), blk, 0, st, (const uint2*)pair, (const int32_t*)a.rown, m, T, depth, mei,
                       nodes);
    // the selection of the channel: its depth keys through the first row of both halves of `keys`
    u64* dsorted = a.keys + (int64_t)(a.group > 1 ? a.group : 1) * m;
    hipLaunchKernelGGL(erpl_depth_dkeys, dim3((unsigned)nb), blk, 0, st, (const double*)depth, (const int32_t*)nodes, m, keys_in);
    e = rocprim::radix_sort_keys(a.temp, temp_bytes, keys_in, dsorted, (size_t)m, 0, 64, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(erpl_depth_select, dim3(1), blk, 0, st, (const double*)depth, (const int32_t*)nodes, m, (const u64*)dsorted, a.central,
                       a.chan + c);
  }
  hipLaunchKernelGGL(erpl_depth_envelope, dim3((unsigned)(C * T)), blk, 0, st, a);
  hipLaunchKernelGGL(erpl_depth_outliers, dim3((unsigned)nb, (unsigned)C), blk, 0, st, a);
  hipLaunchKernelGGL(erpl_depth_whiskers, dim3((unsigned)(C * T)), blk, 0, st, a);
  return (int)hipGetLastError();
}
