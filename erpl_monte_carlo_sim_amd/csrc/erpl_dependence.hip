// erpl_dependence.hip — the device passes of erpl_mc_dependence: given-data sensitivity of an ordinary run (the variance
// share eta^2 with its main-effect curve, Borgonovo's delta, the PAWN Kolmogorov-Smirnov statistics, the mutual
// information), each measure next to its null distribution from cyclic re-pairings.  The population bytes come from the
// first pass of erpl_correlation.hip and are compacted by the select of erpl_bootstrap.hip; what is here works on the
// dense population of m members.
//
//   gather       the requested rows, dense: yd[j][d]
//   classes      per variable: (key_of_tied, dense index) pairs, rocPRIM's radix sort (stable: equal keys stay in dense
//                order), then every sorted position finds its run of equal keys (run_of_key, the rank step of
//                erpl_correlation.hip) and writes the class byte ((first + last + 1) K) div (2 m) of its member: 2 rank - 1 is
//                first + last + 1.  The cell bytes of a row are then extended to 2 m + 32 bytes (byte k = member k mod m).
//   class stats  per factor, while its sorted indices are still there: workgroup (c, j) finds the sorted positions of class
//                c by bisection on the class bytes (they ascend with the position), thread t sums y of the members t,
//                t + 256, .. in sorted order, the fold of erpl_stat_device.h, then the centred squares in a second pass.
//   tables       the hot pass: one workgroup per table (shift p or the run itself, factor, row), (1 + P) F R of them.  A
//                thread takes 16 consecutive members per step: one 16-byte load of class bytes, the 16 cell bytes at d + s
//                from two loads that need 4-byte alignment only (the extension removes the wrap, v_alignbyte the s mod 4),
//                16 integer LDS atomics into the M x H table (at most 16 KB).  The measures are formed in place: the
//                margins by one thread per class / cell, delta_num and the KS maxima in 64-bit integers, mi over the cells
//                of a thread in ascending order, one fold.  A null table never leaves LDS.
// Grids are functions of (m, F, R, M, H, P) alone; integer adds commute and every floating-point sum has a fixed order: the
// same bits in every call.  No floating-point atomics.  Compiled with -ffp-contract=off like its siblings: the quotients
// of delta and KS carry the bits of the host formulae.
#include <rocprim/device/device_radix_sort.hpp>

#include "erpl_philox.h"
#include "erpl_stat_device.h"

namespace {

constexpr int kMaxCells = ERPL_DEP_MAX_CLASSES * ERPL_DEP_MAX_CELLS;   // 4096 counters: 16 KB
constexpr int kChunk = 16;                                             // members per thread and step of the table pass

// four words that are 4-byte aligned only: one global_load_dwordx4 all the same
struct __attribute__((packed, aligned(4))) Words4 {
  uint32_t w[4];
};

// ---- gather
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dep_gather(const ErplDepArgs a) {
  const int j = blockIdx.y;
  const int64_t m = a.m, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ v = a.var[a.n_factors + j];
  const uint32_t* __restrict__ src = a.src;
  double* __restrict__ y = a.yd[j];
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m; d += stride) y[d] = v[src[d]];
}

// ---- classes
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dep_keys(const int64_t m, const double* __restrict__ x,
                                                                const uint32_t* __restrict__ src, u64* __restrict__ keys,
                                                                uint32_t* __restrict__ idx) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m; d += stride) {
    keys[d] = key_of_tied(x[src[d]]);
    idx[d] = (uint32_t)d;
  }
}

// keys / idx: sorted.  K classes; cls[d] of every member d.
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dep_assign(const int64_t m, const u64* __restrict__ keys,
                                                                  const uint32_t* __restrict__ idx, const int K,
                                                                  uint8_t* __restrict__ cls) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t p = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; p < m; p += stride) {
    int64_t first, last;
    run_of_key(keys, p, m, &first, &last);
    cls[idx[p]] = (uint8_t)(((first + last + 1) * K) / (2 * m));   // first + last + 1 <= 2 m - 1: below K
  }
}

// cell byte k = the cell of member k mod m, for m <= k < 2 m + 32 (reads below m, writes from m on)
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dep_extend(const int64_t m, uint8_t* __restrict__ cls) {
  const int64_t total = m + 32, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; e < total; e += stride) cls[m + e] = cls[(m + e) % m];
}

// ---- class stats of factor f: workgroup (c, j).  idx: the factor's sorted dense indices.
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dep_class_stats(const ErplDepArgs a, const int f,
                                                                       const uint32_t* __restrict__ idx) {
  __shared__ uint32_t s_bound[2];
  __shared__ double s_mean;
  const int tid = threadIdx.x, c = blockIdx.x, j = blockIdx.y;
  const uint32_t m = a.m;
  const uint8_t* __restrict__ xc = a.xc + (size_t)f * a.x_stride;
  if (tid < 2) {   // the first sorted position whose class is >= c + tid
    const int want = c + tid;
    uint32_t lo = 0u, hi = m;   // the class of every position below lo is < want, of every one from hi on >= want
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if ((int)xc[idx[mid]] < want) lo = mid + 1u; else hi = mid;
    }
    s_bound[tid] = lo;
  }
  __syncthreads();
  const uint32_t first = s_bound[0], cnt = s_bound[1] - first;
  double* __restrict__ out = a.cstat + (((size_t)j * a.n_factors + f) * a.classes + c) * 6;
  if (cnt == 0u) {   // (uniform)
    if (tid < 6) out[tid] = tid == 0 ? 0.0 : (double)NAN;
    return;
  }
  const double* __restrict__ y = a.yd[j];
  double acc = 0.0;
  for (uint32_t k = tid; k < cnt; k += ERPL_ANA_BLOCK) acc += y[idx[first + k]];
  block_fold<Add>(acc);
  if (tid == 0) s_mean = acc / (double)cnt;
  __syncthreads();
  const double mean = s_mean;
  double ss = 0.0;
  for (uint32_t k = tid; k < cnt; k += ERPL_ANA_BLOCK) {
    const double dev = y[idx[first + k]] - mean;
    ss += dev * dev;
  }
  block_fold_again<Add>(ss);
  if (tid == 0) {
    const double* __restrict__ x = a.var[f];
    out[0] = (double)cnt;
    out[1] = mean;
    out[2] = ss;
    out[3] = x[a.src[idx[first]]];
    out[4] = x[a.src[idx[first + cnt - 1u]]];
    out[5] = x[a.src[idx[first + (cnt - 1u) / 2u]]];
  }
}

// ---- tables
// one pair of class bytes into the table; the mask keeps the add inside the table whatever the bytes are
__device__ __forceinline__ void dep_count(unsigned int* table, const int H, const uint32_t xb, const uint32_t yb) {
  atomicAdd(&table[(xb * (uint32_t)H + yb) & (uint32_t)(kMaxCells - 1)], 1u);
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dep_tables(const ErplDepArgs a) {
  __shared__ unsigned int s_t[kMaxCells];
  __shared__ long long s_n[ERPL_DEP_MAX_CLASSES], s_col[ERPL_DEP_MAX_CELLS];
  __shared__ double s_ks[ERPL_DEP_MAX_CLASSES], s_sorted[ERPL_DEP_MAX_CLASSES];
  const int tid = threadIdx.x, M = a.classes, H = a.cells, cells = M * H;
  const int f = blockIdx.y, j = blockIdx.z, pair = j * a.n_factors + f;
  const uint32_t m = a.m;
  uint32_t s = 0u;   // the shift: 0 for the run itself (blockIdx.x == 0), else s_p of p = blockIdx.x - 1 in 1 .. m - 1
  if (blockIdx.x > 0) {
    const uint32_t p = blockIdx.x - 1u;
    uint64_t A, B;
    erpl_boot_pair(a.seed, 0u, (uint64_t)(p >> 1), &A, &B);
    s = 1u + (uint32_t)erpl_boot_index((p & 1u) ? B : A, (uint64_t)(m - 1u));
  }
  for (int k = tid; k < cells; k += ERPL_ANA_BLOCK) s_t[k] = 0u;
  __syncthreads();

  const uint8_t* __restrict__ x = a.xc + (size_t)f * a.x_stride;
  const uint8_t* __restrict__ y = a.yext + (size_t)j * a.y_stride;
  const uint32_t byte_shift = s & 3u;   // d0 is a multiple of 16: the same for every step
  for (uint32_t d0 = (uint32_t)tid * kChunk; d0 < m; d0 += ERPL_ANA_BLOCK * kChunk) {
    const uint4 xv = *reinterpret_cast<const uint4*>(x + d0);   // inside the row's stride; bytes from m on are not used
    const uint8_t* yb = y + ((d0 + s) & ~3u);                    // d0 + s <= 2 m - 2: the 20 bytes end below 2 m + 32
    const Words4 lo = *reinterpret_cast<const Words4*>(yb);
    const uint32_t hi = *reinterpret_cast<const uint32_t*>(yb + 16);
    const uint32_t xw[4] = {xv.x, xv.y, xv.z, xv.w};
    const uint32_t yw[4] = {__builtin_amdgcn_alignbyte(lo.w[1], lo.w[0], byte_shift),
                            __builtin_amdgcn_alignbyte(lo.w[2], lo.w[1], byte_shift),
                            __builtin_amdgcn_alignbyte(lo.w[3], lo.w[2], byte_shift),
                            __builtin_amdgcn_alignbyte(hi, lo.w[3], byte_shift)};
    if (d0 + kChunk <= m) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int b = 0; b < 4; ++b) dep_count(s_t, H, (xw[i] >> (8 * b)) & 0xffu, (yw[i] >> (8 * b)) & 0xffu);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (d0 + (uint32_t)(4 * i + b) < m) dep_count(s_t, H, (xw[i] >> (8 * b)) & 0xffu, (yw[i] >> (8 * b)) & 0xffu);
    }
  }
  __syncthreads();

  // the margins: thread c the row sum of class c, thread 64 + h the column sum of cell h
  if (tid < M) {
    long long sum = 0;
    for (int h = 0; h < H; ++h) sum += (long long)s_t[tid * H + h];
    s_n[tid] = sum;
  } else if (tid >= 64 && tid < 64 + H) {
    long long sum = 0;
    for (int c = 0; c < M; ++c) sum += (long long)s_t[c * H + (tid - 64)];
    s_col[tid - 64] = sum;
  }
  __syncthreads();

  const long long lm = (long long)m;
  const double dm = (double)m;
  if (tid < M) {   // ks_c; -1 marks an empty class
    const long long nc = s_n[tid];
    double ks = -1.0;
    if (nc > 0) {
      long long cum_t = 0, cum_col = 0, most = 0;
      for (int h = 0; h < H; ++h) {
        cum_t += (long long)s_t[tid * H + h];
        cum_col += s_col[h];
        const long long v = lm * cum_t - nc * cum_col;
        const long long av = v < 0 ? -v : v;
        most = av > most ? av : most;
      }
      ks = (double)most / (dm * (double)nc);
    }
    s_ks[tid] = ks;
  }
  // delta_num and mi: thread t takes the cells t per .. t per + per - 1 in ascending order
  const int per = (cells + ERPL_ANA_BLOCK - 1) / ERPL_ANA_BLOCK;
  u64 dnum = 0ull;
  double mi = 0.0;
  for (int cell = tid * per; cell < (tid + 1) * per && cell < cells; ++cell) {
    const int c = cell / H, h = cell - c * H;
    const long long t = (long long)s_t[cell], nc = s_n[c], col = s_col[h];
    const long long v = lm * t - nc * col;
    dnum += (u64)(v < 0 ? -v : v);
    if (t > 0) mi += ((double)t / dm) * log(((double)t * dm) / ((double)nc * (double)col));
  }
  block_fold<Add, Add>(dnum, mi);   // its barrier also puts s_ks in front of thread 0

  if (blockIdx.x == 0) {   // the table of the run itself is an output
    long long* __restrict__ tab = a.tab + (size_t)pair * cells;
    for (int k = tid; k < cells; k += ERPL_ANA_BLOCK) tab[k] = (long long)s_t[k];
  }
  if (tid != 0) return;
  double* ks = s_sorted;   // the non-empty classes, ascending (insertion: at most 64)
  int used = 0;
  for (int c = 0; c < M; ++c) {
    const double v = s_ks[c];
    if (v < 0.0) continue;
    int at = used++;
    while (at > 0 && ks[at - 1] > v) { ks[at] = ks[at - 1]; --at; }
    ks[at] = v;
  }
  int cells_used = 0;
  for (int h = 0; h < H; ++h) cells_used += s_col[h] > 0 ? 1 : 0;
  const double out[4] = {(double)dnum / ((2.0 * dm) * dm), ks[used - 1],
                         (used & 1) ? ks[used / 2] : (ks[used / 2 - 1] + ks[used / 2]) / 2.0, mi};
  if (blockIdx.x == 0) {
    ErplDepEst& e = a.work->est[pair];
    e.delta_num = (long long)dnum;
    e.classes_used = used;
    e.cells_used = cells_used;
    for (int k = 0; k < 4; ++k) e.v[k] = out[k];
  } else {
    double* __restrict__ nul = a.null + (size_t)pair * 4 * (size_t)a.shifts + (blockIdx.x - 1u);
    for (int k = 0; k < 4; ++k) nul[(size_t)k * (size_t)a.shifts] = out[k];
  }
}

}  // namespace

int erpl_launch_dep_classes(const ErplDepArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t m = (int64_t)a.m;
  const int nb = grid_of(m), F = a.n_factors;
  hipLaunchKernelGGL(erpl_dep_gather, dim3(nb, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a);
  for (int v = 0; v < F + a.n_rows; ++v) {
    hipLaunchKernelGGL(erpl_dep_keys, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, m, a.var[v], a.src, a.keys, a.idx);
    size_t bytes = a.temp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(a.temp, bytes, a.keys, a.keys + m, a.idx, a.idx + m, (size_t)m, 0, 64, st);
    if (e != hipSuccess) return (int)e;
    uint8_t* cls = v < F ? a.xc + (size_t)v * a.x_stride : a.yext + (size_t)(v - F) * a.y_stride;
    hipLaunchKernelGGL(erpl_dep_assign, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, m, a.keys + m, a.idx + m, v < F ? a.classes : a.cells,
                       cls);
    if (v < F)
      hipLaunchKernelGGL(erpl_dep_class_stats, dim3(a.classes, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a, v, a.idx + m);
    else
      hipLaunchKernelGGL(erpl_dep_extend, dim3(grid_of(m + 32)), dim3(ERPL_ANA_BLOCK), 0, st, m, cls);
  }
  return (int)hipGetLastError();
}

int erpl_launch_dep_tables(const ErplDepArgs& a, void* stream) {
  const int nulls = a.m >= 2u ? a.shifts : 0;   // no re-pairing of a single member
  hipLaunchKernelGGL(erpl_dep_tables, dim3(1 + nulls, a.n_factors, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
