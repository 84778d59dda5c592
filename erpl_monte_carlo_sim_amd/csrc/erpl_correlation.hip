// erpl_correlation.hip — the device passes of erpl_mc_correlation: which input dispersion drives which outcome.  The
// reference only records parameter_ranges_observed; this is Pearson / Spearman correlation between [F][n] factor rows
// and rows of the [16][n] summary, next to erpl_mc_analyze.
//
//   population   one pass over the V rows: a byte per sample (0 = mask byte 0 and every variable finite) and the three
//                counts (ballots, 64-bit integer atomics)
//   moments      per variable: sum / min / max over the population, partials per workgroup, the fixed order of
//                erpl_stat_device.h
//   gram         the hot pass: V (V + 1) / 2 centred cross-product sums.  A workgroup stages a tile of ERPL_CORR_TILE
//                samples x V centred values in LDS; a thread owns one 4 x 4 block of the upper triangle and every
//                `slices`-th sample of the tile, 16 running sums in registers, accumulated in sample order; the slices
//                are added in order through LDS, the workgroups' partials by one small kernel in workgroup order
//   ranks        per variable: order-preserving keys (samples outside the population get the largest key), rocPRIM's
//                radix sort of (key, sample index), then every sorted position finds the ends of its run of equal keys
//                by galloping + bisection and scatters first + (len + 1) / 2 to its sample
// Grids and tiles are functions of n and V alone, every floating-point sum has a fixed order (the moments: the one of
// erpl_stat_device.h; the Gram sums: their own, above): the same bits in every call.  No floating-point atomics.
// Compiled with -ffp-contract=off like its siblings: x - mean and the products are rounded as the two-pass NumPy formula
// rounds them (plain fp64 vector multiplies and adds, no MFMA).
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "erpl_stat_device.h"

namespace {

constexpr int kStride = ERPL_CORR_NB * 4 + 2;   // doubles per staged sample: 16-byte aligned rows, spread over the banks

// ---- population: the byte of every sample and the three counts
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corr_population(const ErplCorrArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  u64 cnt[3] = {0ull, 0ull, 0ull};   // in, masked, non-finite: uniform over the wave
  for (int64_t base = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    int why = -1;
    if (i < n) {
      why = (a.mask && a.mask[i] != 0) ? 1 : 0;
      if (why == 0)
        for (int v = 0; v < a.n_vars; ++v)
          if (!finite_bits(a.var[v][i])) why = 2;
      a.pop[i] = (uint8_t)why;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) cnt[k] += __popcll(__ballot(why == k));
  }
  const u64 s = counters_fold(cnt);
  if (threadIdx.x < 3 && s) atomicAdd(&a.work->out.counter[threadIdx.x], s);
}

// ---- first moments of variable blockIdx.y over the population
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corr_moments(const ErplCorrArgs a) {
  const int v = blockIdx.y;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.var[v];
  const uint8_t* __restrict__ pop = a.pop;
  double sum = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < n; i += stride) {
    if (pop[i] == 0) {
      const double val = x[i];
      sum += val;
      mn = val < mn ? val : mn;
      mx = val > mx ? val : mx;
    }
  }
  block_fold<Add, Min, Max>(sum, mn, mx);
  if (threadIdx.x == 0) {
    a.work->psum[v][blockIdx.x] = sum;
    a.work->pmin[v][blockIdx.x] = mn;
    a.work->pmax[v][blockIdx.x] = mx;
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corr_finish_moments(const ErplCorrArgs a, const int nb) {
  const int v = blockIdx.x;
  ErplCorrWork* w = a.work;
  double sum = thread_partials<Add>(w->psum[v], nb);
  double mn = thread_partials<Min>(w->pmin[v], nb), mx = thread_partials<Max>(w->pmax[v], nb);
  block_fold<Add, Min, Max>(sum, mn, mx);
  if (threadIdx.x == 0) {
    const double c = (double)w->out.counter[0];
    w->out.mean[v] = sum / c;   // NaN for an empty population; the host reports every double of it as NaN
    w->out.vmin[v] = mn;
    w->out.vmax[v] = mx;
    w->rank_mean[v] = (c + 1.0) * 0.5;
  }
}

// ---- gram: the centred cross-product sums of this workgroup's tiles, as a blocked upper triangle
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corr_gram(const ErplCorrArgs a, const int which) {
  // the staged tile; afterwards the 16 sums of every thread (256 * 16 doubles fit)
  __shared__ __attribute__((aligned(16))) double s_c[ERPL_CORR_TILE * kStride];
  static_assert(ERPL_CORR_TILE * kStride >= ERPL_ANA_BLOCK * 16, "the slice reduction reuses the tile");
  static_assert(ERPL_ANA_BLOCK % ERPL_CORR_TILE == 0, "a thread stages one sample of the tile");
  const int V = a.n_vars, nbk = (V + 3) / 4, nblk = nbk * (nbk + 1) / 2, vp = nbk * 4;
  const int slices = ERPL_ANA_BLOCK / nblk;   // >= 3: at most 78 blocks
  const int t = threadIdx.x, blk = t % nblk, slice = t / nblk;
  const bool active = slice < slices;
  int bi = 0, bj = blk;
  while (bj >= nbk - bi) { bj -= nbk - bi; ++bi; }
  bj += bi;
  const double* __restrict__ mean = which ? a.work->rank_mean : a.work->out.mean;
  const int64_t n = a.n;
  const int ls = t % ERPL_CORR_TILE, lv = t / ERPL_CORR_TILE;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * ERPL_CORR_TILE; base < n; base += (int64_t)gridDim.x * ERPL_CORR_TILE) {
    __syncthreads();   // the tile before this one has been consumed
    {
      const int64_t i = base + ls;
      const bool use = i < n && a.pop[i] == 0;   // a sample outside the population adds zeros: nothing
      for (int v = lv; v < vp; v += ERPL_ANA_BLOCK / ERPL_CORR_TILE)
        s_c[ls * kStride + v] = (use && v < V) ? a.var[v][i] - mean[v] : 0.0;
    }
    __syncthreads();
    if (active) {
      const int64_t left = n - base;
      const int cnt = left < ERPL_CORR_TILE ? (int)left : ERPL_CORR_TILE;
      for (int s = slice; s < cnt; s += slices) {
        const double* row = s_c + s * kStride;
        double x[4], y[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) { x[p] = row[4 * bi + p]; y[p] = row[4 * bj + p]; }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[p][q] += x[p] * y[q];
      }
    }
  }
  __syncthreads();
  if (active) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) s_c[(slice * nblk + blk) * 16 + p * 4 + q] = acc[p][q];
  }
  __syncthreads();
  for (int k = t; k < nblk * 16; k += ERPL_ANA_BLOCK) {
    double s = 0.0;
    for (int sl = 0; sl < slices; ++sl) s += s_c[sl * nblk * 16 + k];
    a.work->gpart[blockIdx.x][k] = s;
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corr_finish_gram(const ErplCorrArgs a, const int which, const int nwg,
                                                                        const int len) {
  const int k = blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x;
  if (k >= len) return;
  double s = 0.0;
  for (int w = 0; w < nwg; ++w) s += a.work->gpart[w][k];
  a.work->out.gram[which][k] = s;
}

// ---- ranks
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corr_keys(const ErplCorrArgs a, const double* __restrict__ x,
                                                                 u64* __restrict__ keys, uint32_t* __restrict__ idx) {
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < n; i += stride) {
    keys[i] = a.pop[i] == 0 ? key_of_tied(x[i]) : ~0ull;   // no finite double maps to the largest key
    idx[i] = (uint32_t)i;
  }
}

// keys: sorted, the population first.  Position p of a run of equal keys [first, last] (run_of_key in erpl_stat_device.h)
// gets first + (len + 1) / 2 (1-based mid-rank).
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_corr_assign(const ErplCorrArgs a, const u64* __restrict__ keys,
                                                                   const uint32_t* __restrict__ idx, double* __restrict__ rank) {
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const int64_t count = (int64_t)a.work->out.counter[0];
  for (int64_t p = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; p < n; p += stride) {
    const uint32_t i = idx[p];
    if (p >= count) { rank[i] = NAN; continue; }
    int64_t first, last;
    run_of_key(keys, p, count, &first, &last);
    rank[i] = (double)first + (double)(last - first + 2) * 0.5;   // exact: integers and halves below 2^52
  }
}

}  // namespace

int erpl_launch_corr_population(const ErplCorrArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);
  hipError_t e = hipMemsetAsync(&a.work->out.counter[0], 0, sizeof(a.work->out.counter), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(erpl_corr_population, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(erpl_corr_moments, dim3(nb, a.n_vars), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(erpl_corr_finish_moments, dim3(a.n_vars), dim3(ERPL_ANA_BLOCK), 0, st, a, nb);
  return (int)hipGetLastError();
}

int erpl_launch_corr_gram(const ErplCorrArgs& a, int which, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t want = (a.n + ERPL_CORR_TILE - 1) / ERPL_CORR_TILE;
  const int nwg = (int)(want < ERPL_CORR_GRAM_MAX_BLOCKS ? want : ERPL_CORR_GRAM_MAX_BLOCKS);
  const int nbk = (a.n_vars + 3) / 4, len = nbk * (nbk + 1) / 2 * 16;
  hipLaunchKernelGGL(erpl_corr_gram, dim3(nwg), dim3(ERPL_ANA_BLOCK), 0, st, a, which);
  hipLaunchKernelGGL(erpl_corr_finish_gram, dim3((len + ERPL_ANA_BLOCK - 1) / ERPL_ANA_BLOCK), dim3(ERPL_ANA_BLOCK), 0, st, a,
                     which, nwg, len);
  return (int)hipGetLastError();
}

int erpl_launch_corr_ranks(const ErplCorrArgs& a, const double* x, double* rank_row, unsigned long long* keys, uint32_t* idx,
                           void* temp, size_t* temp_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)a.n;
  if (!temp) return (int)rocprim::radix_sort_pairs(nullptr, *temp_bytes, keys, keys, idx, idx, n, 0, 64, st);   // sizing only
  const int nb = grid_of(a.n);
  hipLaunchKernelGGL(erpl_corr_keys, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a, x, keys, idx);
  hipError_t e = rocprim::radix_sort_pairs(temp, *temp_bytes, keys, keys + n, idx, idx + n, n, 0, 64, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(erpl_corr_assign, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a, keys + n, idx + n, rank_row);
  return (int)hipGetLastError();
}
