// erpl_sobol.hip — the device passes of erpl_mc_sobol: first-order and total-effect indices of a pick-freeze design and
// their bootstrap, next to erpl_mc_bootstrap.  The population bytes of every requested row come from the first pass of
// erpl_correlation.hip and are compacted by the select of erpl_bootstrap.hip; what is here works on the result.
//
//   records      once per call: rec[r][d][0 .. k + 1] = the k + 2 block values (A, B, AB_0 ..) of dense member d of row r,
//                contiguous - a draw is ONE read of 24 - 272 bytes instead of k + 2 reads n_base * 8 bytes apart.
//   estimates    the estimators over the population itself: two passes over the grid of the analysis calls (a function of
//                m alone), thread by thread in index order, the partials of the workgroups folded by one workgroup per sum.
//   replicate    the hot kernel: one workgroup of ERPL_ANA_BLOCK threads per (replicate, row).  Its m draws are never
//                stored: every sweep regenerates them from the counter, with the Philox pairs shared between neighbouring
//                threads as in erpl_boot_replicate.  Thread t takes the draws t, t + 256, .. in order.  Sweep 1 sums yA,
//                then yB, of every drawn record; sweep 2 the centred squares and, per factor, (yB - f0) d_i and d_i d_i
//                with d_i = yAB_i - yA.  Sweep 2 runs once per chunk of ERPL_SOBOL_CHUNK factors: a thread carries
//                1 + 2 * 8 running sums whatever k is (k = 32 in one sweep would be 65 sums, 130 registers of sums alone,
//                and one wave per SIMD on a kernel that lives on the latency of its gathers); the price is one more
//                regeneration of the draws per chunk.
// The arithmetic of a record is written once (sobol_first, sobol_second) and used by the estimates with the identity in
// place of the draw.  Sums are folded in the fixed order of erpl_stat_device.h; no floating-point atomics: the same bits
// in every call, and replicate b does not depend on how many replicates there are.  Compiled with -ffp-contract=off like
// its siblings.
#include <hip/hip_runtime.h>

#include <utility>

#include "erpl_philox.h"
#include "erpl_stat_device.h"

namespace {

constexpr int kChunk = ERPL_SOBOL_CHUNK;
template <size_t>
using AddAt = Add;

// sweep 1 of one record
__device__ __forceinline__ void sobol_first(const double* __restrict__ rec, double& acc) {
  acc += rec[0];
  acc += rec[1];
}

// sweep 2 of one record for the factors c0 .. c0 + nf - 1 (nf <= kChunk; the centred squares with the first chunk)
__device__ __forceinline__ void sobol_second(const double* __restrict__ rec, const int c0, const int nf, const double f0,
                                             double& v, double (&s1)[kChunk], double (&st)[kChunk]) {
  const double ya = rec[0], yb = rec[1];
  double y[kChunk];
#pragma unroll
  for (int u = 0; u < kChunk; ++u) y[u] = u < nf ? rec[2 + c0 + u] : ya;   // never read past the record
  const double cb = yb - f0;
  if (c0 == 0) {
    const double ca = ya - f0;
    v += ca * ca;
    v += cb * cb;
  }
#pragma unroll
  for (int u = 0; u < kChunk; ++u)
    if (u < nf) {
      const double d = y[u] - ya;
      s1[u] += cb * d;
      st[u] += d * d;
    }
}

// the 1 + 2 kChunk sums of a chunk through ONE fold (valid in thread 0); every call is guarded: the kernels loop over it
template <size_t... I>
__device__ __forceinline__ void fold_chunk(double& v, double (&s1)[kChunk], double (&st)[kChunk], std::index_sequence<I...>) {
  block_fold_again<Add, AddAt<I>..., AddAt<I>...>(v, s1[I]..., st[I]...);
}

// ---- records
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_sobol_records(const ErplSobolArgs a) {
  const int r = blockIdx.y;
  const int64_t K2 = a.k + 2, total = (int64_t)a.m[r] * K2;   // < 2^31
  const int nb = grid_of(total);
  if ((int)blockIdx.x >= nb) return;
  const double* __restrict__ v = a.var[r];
  const uint32_t* __restrict__ src = a.src[r];
  double* __restrict__ rec = a.rec[r];
  const int64_t stride = (int64_t)nb * ERPL_ANA_BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; e < total; e += stride) {
    const int64_t d = e / K2, b = e - d * K2;
    rec[e] = v[b * a.n_base + (int64_t)src[d]];
  }
}

// ---- estimates: second = 0: slot 0 (the sum of yA and yB); second = 1: the slots 1 .. 1 + 2 k, centred on out.f0
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_sobol_estimate(const ErplSobolArgs a, const int second) {
  const int r = blockIdx.y, tid = threadIdx.x, k = a.k, K2 = k + 2;
  const int64_t m = a.m[r];
  const int nb = grid_of(m);
  if ((int)blockIdx.x >= nb) return;   // (uniform over the workgroup; an empty population has no workgroup at all)
  const double* __restrict__ rec = a.rec[r];
  double (*part)[ERPL_ANA_MAX_BLOCKS] = a.work->part[r];
  const int64_t first = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + tid, stride = (int64_t)nb * ERPL_ANA_BLOCK;
  if (!second) {
    double acc = 0.0;
    for (int64_t d = first; d < m; d += stride) sobol_first(rec + d * K2, acc);
    block_fold<Add>(acc);
    if (tid == 0) part[0][blockIdx.x] = acc;
    return;
  }
  const double f0 = a.work->out.f0[r];
  for (int c0 = 0; c0 < k; c0 += kChunk) {
    const int nf = k - c0 < kChunk ? k - c0 : kChunk;
    double v = 0.0, s1[kChunk], st[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; ++u) s1[u] = st[u] = 0.0;
    for (int64_t d = first; d < m; d += stride) sobol_second(rec + d * K2, c0, nf, f0, v, s1, st);
    fold_chunk(v, s1, st, std::make_index_sequence<kChunk>{});
    if (tid == 0) {
      if (c0 == 0) part[1][blockIdx.x] = v;
#pragma unroll
      for (int u = 0; u < kChunk; ++u)
        if (u < nf) {
          part[2 + c0 + u][blockIdx.x] = s1[u];
          part[2 + k + c0 + u][blockIdx.x] = st[u];
        }
    }
  }
}

// workgroup (x, r) folds the partials of slot slot0 + x of row r
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_sobol_estimate_finish(const ErplSobolArgs a, const int slot0) {
  const int r = blockIdx.y, slot = slot0 + blockIdx.x;
  const int64_t m = a.m[r];
  double v = thread_partials<Add>(a.work->part[r][slot], grid_of(m));
  block_fold<Add>(v);
  if (threadIdx.x == 0) {
    a.work->out.sum[r][slot] = v;
    if (slot == 0) a.work->out.f0[r] = v / (2.0 * (double)m);   // NaN for an empty population: the host reports NaN
  }
}

// ---- replicate
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_sobol_replicate(const ErplSobolArgs a) {
  __shared__ double s_f0;
  const int tid = threadIdx.x, r = blockIdx.y, k = a.k, ns = 2 + 2 * k;
  const size_t K2 = (size_t)(k + 2), B = (size_t)a.replicates;
  const uint32_t b = blockIdx.x, m = a.m[r];
  double* __restrict__ out = a.rep + (size_t)(r * ns) * B + b;   // statistic s at out[s * B]
  if (m == 0u) {   // (uniform) every replicate of an empty population is NaN
    for (int s = tid; s < ns; s += ERPL_ANA_BLOCK) out[(size_t)s * B] = (double)NAN;
    return;
  }
  const double* __restrict__ rec = a.rec[r];
  const double dm = (double)m, dm2 = 2.0 * dm;
  const bool even = (tid & 1) == 0;
  double V = 0.0;   // thread 0, from the first chunk on
  // sweep 0: the mean; then one sweep per chunk of factors, c0 = its first factor
  for (int c0 = -kChunk; c0 < k; c0 += kChunk) {
    const bool mean_sweep = c0 < 0;
    const int nf = k - c0 < kChunk ? k - c0 : kChunk;
    const double f0 = mean_sweep ? 0.0 : s_f0;
    double acc = 0.0, s1[kChunk], st[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; ++u) s1[u] = st[u] = 0.0;
    // `base` is uniform over the workgroup: every lane takes part in every shuffle
    for (uint32_t base = 0; base < m; base += 2 * ERPL_ANA_BLOCK) {
      const uint32_t t1 = base + (uint32_t)tid, t2 = t1 + ERPL_ANA_BLOCK;   // this thread's draws, in this order
      const uint32_t mine = even ? t1 : t2;   // the draw whose Philox pair this thread computes
      uint64_t A, Bv;
      erpl_boot_pair(a.seed, b, (uint64_t)(mine >> 1), &A, &Bv);
      const uint32_t dA = (uint32_t)erpl_boot_index(A, m), dB = (uint32_t)erpl_boot_index(Bv, m);
      // even thread: A is its draw t1, B the draw t1 + 1 of its odd neighbour; odd thread: B is its draw t2, A the draw
      // t2 - 1 of its even neighbour
      const uint32_t got = (uint32_t)__shfl_xor((int)(even ? dB : dA), 1);
      const uint32_t d1 = even ? dA : got, d2 = even ? got : dB;   // both below m: a record of the table
      const bool v1 = t1 < m, v2 = t2 < m;
      if (mean_sweep) {
        if (v1) sobol_first(rec + (size_t)d1 * K2, acc);
        if (v2) sobol_first(rec + (size_t)d2 * K2, acc);
      } else {
        if (v1) sobol_second(rec + (size_t)d1 * K2, c0, nf, f0, acc, s1, st);
        if (v2) sobol_second(rec + (size_t)d2 * K2, c0, nf, f0, acc, s1, st);
      }
    }
    if (mean_sweep) {
      block_fold<Add>(acc);
      if (tid == 0) {
        s_f0 = acc / dm2;
        out[0] = acc / dm2;
      }
      __syncthreads();   // the mean is there
      continue;
    }
    fold_chunk(acc, s1, st, std::make_index_sequence<kChunk>{});
    if (tid == 0) {
      if (c0 == 0) {
        V = acc / dm2;
        out[B] = V;
      }
      const bool flat = V == 0.0;   // no variance to share out
#pragma unroll
      for (int u = 0; u < kChunk; ++u)
        if (u < nf) {
          out[(size_t)(2 + c0 + u) * B] = flat ? (double)NAN : (s1[u] / dm) / V;
          out[(size_t)(2 + k + c0 + u) * B] = flat ? (double)NAN : (st[u] / dm2) / V;
        }
    }
  }
}

// the widest grid the rows ask for: workgroups beyond a row's own grid leave at once
int widest_grid(const ErplSobolArgs& a, int64_t per_member) {
  int nb = 0;
  for (int r = 0; r < a.n_rows; ++r) {
    const int g = grid_of((int64_t)a.m[r] * per_member);
    nb = g > nb ? g : nb;
  }
  return nb;
}

}  // namespace

int erpl_launch_sobol_records(const ErplSobolArgs& a, void* stream) {
  const int nb = widest_grid(a, a.k + 2);
  if (nb > 0) hipLaunchKernelGGL(erpl_sobol_records, dim3(nb, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int erpl_launch_sobol_estimates(const ErplSobolArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = widest_grid(a, 1);
  if (nb > 0) hipLaunchKernelGGL(erpl_sobol_estimate, dim3(nb, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a, 0);
  hipLaunchKernelGGL(erpl_sobol_estimate_finish, dim3(1, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a, 0);
  if (nb > 0) hipLaunchKernelGGL(erpl_sobol_estimate, dim3(nb, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a, 1);
  hipLaunchKernelGGL(erpl_sobol_estimate_finish, dim3(1 + 2 * a.k, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a, 1);
  return (int)hipGetLastError();
}

int erpl_launch_sobol_replicates(const ErplSobolArgs& a, void* stream) {
  hipLaunchKernelGGL(erpl_sobol_replicate, dim3(a.replicates, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
