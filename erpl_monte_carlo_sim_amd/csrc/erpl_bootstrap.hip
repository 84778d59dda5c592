// erpl_bootstrap.hip — the device passes of erpl_mc_bootstrap: how sure the statistics of a finished run are.  The
// reference prints point estimates only (monte_carlo.py:400-473); this is the non-parametric bootstrap of mean, standard
// deviation and quantiles of up to four rows, next to erpl_mc_analyze.
//
//   prepare      once per call: the population bytes of erpl_correlation.hip's first pass are compacted in sample order
//                (rocPRIM select -> src[d], the sample of dense member d), the rows gathered to x[r][d], and per row
//                (key_of_signed(x), d) sorted with rocPRIM's radix sort: sorted[r][p] and pos[r][d], the sorted position
//                of member d.  Ties need no care: equal keys are equal values.
//   replicate    the hot kernel: one workgroup of ERPL_ANA_BLOCK threads owns replicate b from start to end.  Its m draws
//                are never stored: every sweep regenerates them from the counter (erpl_philox.h, one Philox call per two
//                draws).  Thread t takes the draws t, t + 256, ..: the even thread of a pair of threads computes the
//                Philox pair of their first draws, the odd one that of their second draws, and they swap the halves.
//                Per row: sweep 1 sums, sweep 2 sums the centred squares, and the order statistics come from most-
//                significant-digit radix selection on the 32-bit sorted POSITIONS pos[r][d] - ceil(bits(m - 1) / 8)
//                sweeps of one 8-bit digit, the first two riding on the moment sweeps.  Histograms (one per group of
//                targets that still share a prefix, LDS integer atomics, the whole-wave-in-one-bin shortcut) and the
//                scan between the sweeps are those of erpl_ana_histogram / erpl_ana_scan, kept inside the workgroup.
// The summary over the replicates and the estimates over the population are erpl_launch_row_stats (erpl_analysis.hip).
// Sums are accumulated per thread in draw order and folded in the fixed order of erpl_stat_device.h; integer adds commute:
// the same bits in every call, and replicate b does not depend on how many replicates there are.  No floating-point
// atomics.  Compiled with -ffp-contract=off like its siblings.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "erpl_philox.h"
#include "erpl_stat_device.h"

namespace {

struct InPopulation {
  __host__ __device__ bool operator()(const uint8_t& why) const { return why == 0; }
};

// ---- prepare
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_boot_gather(const ErplBootPrep p) {
  const int r = blockIdx.y;
  const int64_t m = p.m, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ v = p.var[r];
  const uint32_t* __restrict__ src = p.src;
  double* __restrict__ x = p.x[r];
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m; d += stride) x[d] = v[src[d]];
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_boot_keys(const int64_t m, const double* __restrict__ x,
                                                                 u64* __restrict__ keys, uint32_t* __restrict__ idx) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m; d += stride) {
    keys[d] = key_of_signed(x[d]);
    idx[d] = (uint32_t)d;
  }
}

// keys / idx: sorted.  The value back from its key (the inverse of key_of_signed), and where every member went.
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_boot_place(const int64_t m, const u64* __restrict__ keys,
                                                                  const uint32_t* __restrict__ idx, double* __restrict__ sorted,
                                                                  uint32_t* __restrict__ pos) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t p = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; p < m; p += stride) {
    const u64 k = keys[p];
    sorted[p] = __longlong_as_double((long long)(k ^ ((k >> 63) ? (1ull << 63) : ~0ull)));
    pos[idx[p]] = (uint32_t)p;
  }
}

// ---- replicate
// One digit of one draw into the histograms of the groups whose prefix its position shares.  Every lane of the wave calls
// it (ballots); `valid` is false for a lane without a draw.
__device__ __forceinline__ void boot_count(unsigned int (*hist)[ERPL_ANA_BINS], const uint32_t* gprefix, const int* lead,
                                           const int nlead, const uint32_t p, const bool valid, const uint32_t above,
                                           const int shift) {
  const unsigned int digit = (p >> shift) & (ERPL_ANA_BINS - 1);
  for (int g = 0; g < nlead; ++g) {
    const bool hit = valid && ((p ^ gprefix[g]) & above) == 0u;
    const u64 mask = __ballot(hit);
    if (mask == 0ull) continue;
    // a group that has narrowed to one bin puts a whole wave there: one add of the lane count
    const int lead_lane = __ffsll((long long)mask) - 1;
    const unsigned int d0 = (unsigned int)__shfl((int)digit, lead_lane);
    if (__ballot(hit && digit != d0) == 0ull) {
      if ((int)(threadIdx.x & 63) == lead_lane) atomicAdd(&hist[lead[g]][d0], (unsigned int)__popcll(mask));
    } else if (hit) {
      atomicAdd(&hist[lead[g]][digit], 1u);
    }
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_boot_replicate(const ErplBootArgs a) {
  __shared__ unsigned int s_hist[ERPL_ANA_TARGETS][ERPL_ANA_BINS];   // 16 KB
  __shared__ uint32_t s_prefix[ERPL_ANA_TARGETS], s_rank[ERPL_ANA_TARGETS], s_gprefix[ERPL_ANA_TARGETS];
  __shared__ int s_leader[ERPL_ANA_TARGETS], s_lead[ERPL_ANA_TARGETS];
  __shared__ int s_nlead;
  __shared__ double s_mean;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t b = blockIdx.x, m = a.m;
  const int nt = 2 * a.n_q, ns = 2 + a.n_q, ndig = a.n_digits;
  const size_t B = (size_t)a.replicates;
  const double dm = (double)m;
  const bool even = (tid & 1) == 0;
  const int sweeps = (nt > 0 && ndig > 2) ? ndig : 2;

  for (int r = 0; r < a.n_rows; ++r) {
    const double* __restrict__ x = a.x[r];
    const double* __restrict__ sorted = a.sorted[r];
    const uint32_t* __restrict__ pos = a.pos[r];
    // every target starts in one group with an empty prefix
    if (tid < ERPL_ANA_TARGETS) { s_prefix[tid] = 0u; s_rank[tid] = a.rank[tid]; s_leader[tid] = 0; }
    if (tid == 0) { s_nlead = nt > 0 ? 1 : 0; s_lead[0] = 0; s_gprefix[0] = 0u; }
    for (int k = tid; k < ERPL_ANA_TARGETS * ERPL_ANA_BINS; k += ERPL_ANA_BLOCK) (&s_hist[0][0])[k] = 0u;
    __syncthreads();
    double mean = 0.0;
    for (int sw = 0; sw < sweeps; ++sw) {
      const bool digit = nt > 0 && sw < ndig;
      const int shift = digit ? 8 * (ndig - 1 - sw) : 0;
      const uint32_t above = shift + 8 >= 32 ? 0u : (~0u << (shift + 8));   // the bits fixed before this sweep
      const int nlead = digit ? s_nlead : 0;
      double acc = 0.0;
      // `base` is uniform over the workgroup: every lane takes part in every shuffle and ballot
      for (uint32_t base = 0; base < m; base += 2 * ERPL_ANA_BLOCK) {
        const uint32_t t1 = base + (uint32_t)tid, t2 = t1 + ERPL_ANA_BLOCK;   // this thread's draws, in this order
        const uint32_t mine = even ? t1 : t2;   // the draw whose Philox pair this thread computes
        uint64_t A, Bv;
        erpl_boot_pair(a.seed, b, (uint64_t)(mine >> 1), &A, &Bv);
        const uint32_t dA = (uint32_t)erpl_boot_index(A, m), dB = (uint32_t)erpl_boot_index(Bv, m);
        // even thread: A is its draw t1, B the draw t1 + 1 of its odd neighbour; odd thread: B is its draw t2, A the draw
        // t2 - 1 of its even neighbour
        const uint32_t got = (uint32_t)__shfl_xor((int)(even ? dB : dA), 1);
        const uint32_t d1 = even ? dA : got, d2 = even ? got : dB;
        const bool v1 = t1 < m, v2 = t2 < m;
        uint32_t p1 = 0u, p2 = 0u;
        if (digit) {
          if (v1) p1 = pos[d1];
          if (v2) p2 = pos[d2];
        }
        if (sw < 2) {
          const double x1 = v1 ? x[d1] : 0.0, x2 = v2 ? x[d2] : 0.0;
          if (sw == 0) {
            if (v1) acc += x1;
            if (v2) acc += x2;
          } else {
            if (v1) { const double c = x1 - mean; acc += c * c; }
            if (v2) { const double c = x2 - mean; acc += c * c; }
          }
        }
        if (digit) {
          boot_count(s_hist, s_gprefix, s_lead, nlead, p1, v1, above, shift);
          boot_count(s_hist, s_gprefix, s_lead, nlead, p2, v2, above, shift);
        }
      }
      if (sw < 2) {
        block_fold_again<Add>(acc);
        if (tid == 0) {
          if (sw == 0) {
            s_mean = acc / dm;
            a.rep[(size_t)(r * ns) * B + b] = acc / dm;
          } else {
            a.rep[(size_t)(r * ns + 1) * B + b] = sqrt(acc / dm);
          }
        }
      }
      __syncthreads();   // the histograms are complete, the mean is there
      mean = s_mean;
      if (!digit) continue;   // uniform
      // wave w scans the histograms of the targets w, w + kWaves, ..: fixes the digit that holds the rank
      for (int t = wave; t < nt; t += kWaves) {
        const unsigned int* h = s_hist[s_leader[t]];
        const uint32_t rank = s_rank[t];
        uint32_t c[4], s = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) { c[k] = h[lane * 4 + k]; s += c[k]; }
        uint32_t incl = s;
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
          if (lane >= off) incl += up;
        }
        uint32_t before = incl - s;
        if (before <= rank && rank < incl) {   // exactly one lane
          int d = 0;
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (rank >= before + c[k] && d == k) { before += c[k]; d = k + 1; }
          s_prefix[t] |= (uint32_t)(lane * 4 + d) << shift;
          s_rank[t] = rank - before;
        }
      }
      __syncthreads();   // every histogram has been read, every prefix is known
      if (tid == 0) {
        int nl = 0;
        for (int t = 0; t < nt; ++t) {
          int lead = t;
          for (int u = t - 1; u >= 0; --u) if (s_prefix[u] == s_prefix[t]) lead = u;
          s_leader[t] = lead;
          if (lead == t) { s_lead[nl] = t; s_gprefix[nl] = s_prefix[t]; ++nl; }
        }
        s_nlead = nl;
      }
      for (int k = tid; k < ERPL_ANA_TARGETS * ERPL_ANA_BINS; k += ERPL_ANA_BLOCK) (&s_hist[0][0])[k] = 0u;
      __syncthreads();
    }
    if (tid < a.n_q) {
      // the selected positions are below m by construction; the clamp keeps a read inside the row whatever happens
      const uint32_t plo = s_prefix[2 * tid] < m ? s_prefix[2 * tid] : m - 1u;
      const uint32_t phi = s_prefix[2 * tid + 1] < m ? s_prefix[2 * tid + 1] : m - 1u;
      const double lo = sorted[plo], hi = sorted[phi];
      a.rep[(size_t)(r * ns + 2 + tid) * B + b] = lo + (hi - lo) * a.frac[tid];
    }
    __syncthreads();   // the selection state is read before the next row resets it
  }
}

}  // namespace

int erpl_boot_temp_bytes(int64_t n, size_t* bytes) {
  size_t sel = 0, srt = 0;
  hipError_t e = rocprim::select(nullptr, sel, rocprim::counting_iterator<uint32_t>(0u),
                                 rocprim::make_transform_iterator((const uint8_t*)nullptr, InPopulation()), (uint32_t*)nullptr,
                                 (unsigned long long*)nullptr, (size_t)n, (hipStream_t)0);
  if (e != hipSuccess) return (int)e;
  e = rocprim::radix_sort_pairs(nullptr, srt, (u64*)nullptr, (u64*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0,
                                64, (hipStream_t)0);
  if (e != hipSuccess) return (int)e;
  *bytes = sel > srt ? sel : srt;
  return 0;
}

int erpl_boot_select_bytes(int64_t n, size_t* bytes) {
  return (int)rocprim::select(nullptr, *bytes, rocprim::counting_iterator<uint32_t>(0u),
                              rocprim::make_transform_iterator((const uint8_t*)nullptr, InPopulation()), (uint32_t*)nullptr,
                              (unsigned long long*)nullptr, (size_t)n, (hipStream_t)0);
}

int erpl_launch_boot_compact(const ErplBootPrep& p, void* stream) {
  size_t bytes = p.temp_bytes;
  return (int)rocprim::select(p.temp, bytes, rocprim::counting_iterator<uint32_t>(0u),
                              rocprim::make_transform_iterator(p.pop, InPopulation()), p.src, p.count, (size_t)p.n,
                              (hipStream_t)stream);
}

int erpl_launch_boot_prepare(const ErplBootPrep& p, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(p.m);
  const size_t m = (size_t)p.m;
  hipLaunchKernelGGL(erpl_boot_gather, dim3(nb, p.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, p);
  for (int r = 0; r < p.n_rows; ++r) {
    hipLaunchKernelGGL(erpl_boot_keys, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, p.m, p.x[r], p.keys, p.idx);
    size_t bytes = p.temp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(p.temp, bytes, p.keys, p.keys + m, p.idx, p.idx + m, m, 0, 64, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(erpl_boot_place, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, p.m, p.keys + m, p.idx + m, p.sorted[r], p.pos[r]);
  }
  return (int)hipGetLastError();
}

int erpl_launch_boot_replicates(const ErplBootArgs& a, void* stream) {
  hipLaunchKernelGGL(erpl_boot_replicate, dim3(a.replicates), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
