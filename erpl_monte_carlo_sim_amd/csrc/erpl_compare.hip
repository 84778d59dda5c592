// erpl_compare.hip — the device passes of erpl_mc_compare: two-sample tests between two runs (Kolmogorov-Smirnov,
// Mann-Whitney, Cramer-von Mises per row, the energy statistic of the impact clouds), each recomputed under P relabellings
// of the pooled members.  The populations come from the first pass of erpl_correlation.hip and the select of
// erpl_bootstrap.hip; what is here works on the N = m_a + m_b pooled dense members (A's, then B's).
//
//   gather       the requested rows and the (x, y) pairs, pooled: val[j][i], xy[i]
//   ranks        per row: (key_of_tied, i) pairs, rocPRIM's radix sort (stable), then every sorted position finds its run of
//                equal keys (run_of_key): sidx[s], the member there, and r2e[s] = 2 r | last-of-its-class << 63.
//   thresholds   one workgroup per permutation p: the m_a-th smallest (key, i) pair by most-significant-digit radix selection
//                over keys that are regenerated in every sweep (erpl_philox.h: draw i of replicate p), eight sweeps of one
//                8-bit digit (select_scan of erpl_stat_device.h), then the index among equal keys (one sweep per tie).
//   bits         replicate q = 0 is the observed labelling (i < m_a), q = p + 1 permutation p.  A wave takes a Philox pair
//                (members 2 j, 2 j + 1) and a word: lane l is replicate 64 word + l, one comparison against its threshold,
//                two ballots, two 64-bit vector stores: bits[i][word].
//   HOT LOOP 1   rank statistics, lane = replicate.  The sorted order of a row is cut into chunks (erpl_cmp_chunks); a wave
//                owns (chunk, word).  It loads 64 positions at a time (sidx, r2e and the member's word: 64 gathers in flight)
//                and hands them round by v_readlane; every lane takes its own bit, carries c_A and folds K with its first
//                position and sign, the sum of 2 r over A and the two sums of (2 r - 2 c)^2 as 128-bit integers.  Pass 1
//                counts the A members per chunk, a scan turns the counts into the c_A a chunk starts from, pass 2 walks, a
//                last kernel folds the chunks in ascending order.  ONLY INTEGERS: no order matters, nothing is rounded.
//   HOT LOOP 2   all pairs, thread = pooled member i, workgroup = (tile of 256 members, slice of sources, word).  The sources
//                of a slice are staged through LDS 256 at a time ((x, y) and the word of their labels) and read back at one
//                address per wave: a broadcast.  d_ij is computed once per word and added under the wave-uniform label bit of
//                source j into 64 accumulators in registers (r_i of every replicate: fma(bit, d, r), bit 0.0 or 1.0 from
//                scalar registers) and into t_i.  Then S_AA takes r_i if i is on side A, S_AB r_i and S_BB t_i - r_i if not;
//                the 256 members are folded per replicate in the fixed order of erpl_stat_device.h (wave tree, waves 0..3),
//                and a last kernel adds the partial sums in ascending (tile, slice) order.
// Grids are functions of (N, P) alone; every fp64 sum has a fixed order: the same bits in every call.  No floating-point
// atomics, vector stores only.  Compiled with -ffp-contract=off like its siblings.
#include <rocprim/device/device_radix_sort.hpp>

#include "erpl_philox.h"
#include "erpl_stat_device.h"

namespace {

constexpr unsigned long long kEnd = 1ull << 63;

// lane k's 64-bit value in every lane (k uniform)
__device__ __forceinline__ u64 word_of_lane(u64 v, int k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k);
  return ((u64)hi << 32) | lo;
}

// ---- gather
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_gather(const ErplCmpArgs a) {
  const int j = blockIdx.y;   // a row, or n_rows: the plane
  const int64_t N = (int64_t)a.N, m_a = (int64_t)a.m_a, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < N; i += stride) {
    const bool in_a = i < m_a;
    const uint32_t s = in_a ? a.src_a[i] : a.src_b[i - m_a];
    if (j < a.n_rows) {
      a.val[j][i] = (in_a ? a.var_a[j] : a.var_b[j])[s];
    } else {
      const double x = (in_a ? a.var_a[a.n_rows] : a.var_b[a.n_rows])[s], y = (in_a ? a.var_a[a.n_rows + 1] : a.var_b[a.n_rows + 1])[s];
      reinterpret_cast<double2*>(a.xy)[i] = make_double2(x, y);
    }
  }
}

// ---- ranks
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_keys(const int64_t N, const double* __restrict__ x, u64* __restrict__ keys,
                                                                uint32_t* __restrict__ idx) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < N; i += stride) {
    keys[i] = key_of_tied(x[i]);
    idx[i] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_ranks(const int64_t N, const u64* __restrict__ keys,
                                                                 const uint32_t* __restrict__ idx, uint32_t* __restrict__ sidx,
                                                                 u64* __restrict__ r2e) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t s = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; s < N; s += stride) {
    int64_t first, last;
    run_of_key(keys, s, N, &first, &last);
    sidx[s] = idx[s];
    r2e[s] = (u64)(first + last + 2) | (s == last ? kEnd : 0ull);   // 2 r = (first + 1) + (last + 1) < 2^33
  }
}

// ---- thresholds: workgroup p -> thr[2 (p + 1)], thr[2 (p + 1) + 1]
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_thresholds(const u64 seed, const u64 N, const u64 m_a, u64* __restrict__ thr) {
  __shared__ unsigned int s_hist[ERPL_ANA_BINS];
  __shared__ u64 s_prefix, s_rank;
  __shared__ unsigned int s_min;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t p = blockIdx.x;
  const u64 pairs = (N + 1) / 2;
  if (tid == 0) { s_prefix = 0ull; s_rank = m_a - 1ull; }
  for (int shift = 56; shift >= 0; shift -= 8) {
    s_hist[tid] = 0u;   // ERPL_ANA_BINS == ERPL_ANA_BLOCK
    __syncthreads();
    const u64 prefix = s_prefix, rank = s_rank;
    const u64 above = shift >= 56 ? 0ull : (~0ull << (shift + 8));
    for (u64 j = tid; j < pairs; j += ERPL_ANA_BLOCK) {
      uint64_t A, B;
      erpl_boot_pair(seed, p, j, &A, &B);
      if (((A ^ prefix) & above) == 0ull) atomicAdd(&s_hist[(A >> shift) & (ERPL_ANA_BINS - 1)], 1u);
      if (2 * j + 1 < N && ((B ^ prefix) & above) == 0ull) atomicAdd(&s_hist[(B >> shift) & (ERPL_ANA_BINS - 1)], 1u);
    }
    __syncthreads();
    if (tid < 64) {
      int digit;
      u64 below;
      if (select_scan(s_hist, rank, lane, &digit, &below)) {
        s_prefix = prefix | ((u64)digit << shift);
        s_rank = rank - below;
      }
    }
    __syncthreads();
  }
  // s_rank + 1 members with the key s_prefix are on side A: the one with the largest index among them, in s_rank + 1 sweeps
  const u64 key = s_prefix, ties = s_rank;
  u64 prev = 0ull;
  for (u64 t = 0; t <= ties; ++t) {
    if (tid == 0) s_min = 0xffffffffu;
    __syncthreads();
    for (u64 j = tid; j < pairs; j += ERPL_ANA_BLOCK) {
      uint64_t A, B;
      erpl_boot_pair(seed, p, j, &A, &B);
      if (A == key && (t == 0 || 2 * j > prev)) atomicMin(&s_min, (unsigned int)(2 * j));
      if (2 * j + 1 < N && B == key && (t == 0 || 2 * j + 1 > prev)) atomicMin(&s_min, (unsigned int)(2 * j + 1));
    }
    __syncthreads();
    prev = (u64)s_min;
    __syncthreads();
  }
  if (tid == 0) {
    thr[2 * ((u64)p + 1)] = key;
    thr[2 * ((u64)p + 1) + 1] = prev;
  }
}

// ---- bits: grid (., wl); the words w0 .. w0 + wl - 1 of every member
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_bits(const u64 seed, const u64 N, const u64 m_a, const int Q, const int w0,
                                                                const int wb, const u64* __restrict__ thr, u64* __restrict__ bits) {
  const int lane = threadIdx.x & 63, word = blockIdx.y;
  const u64 wave = (u64)blockIdx.x * kWaves + (threadIdx.x >> 6), waves = (u64)gridDim.x * kWaves, pairs = (N + 1) / 2;
  const int q = (w0 + word) * 64 + lane;
  const bool valid = q < Q, identity = q == 0;
  const u64 tk = valid && !identity ? thr[2 * (u64)q] : 0ull, ti = valid && !identity ? thr[2 * (u64)q + 1] : 0ull;
  for (u64 j = wave; j < pairs; j += waves) {
    uint64_t A, B;
    erpl_boot_pair(seed, (uint32_t)(q - 1), j, &A, &B);
    const u64 i0 = 2 * j, i1 = i0 + 1;
    const bool l0 = valid && (identity ? i0 < m_a : erpl_cmp_label(A, i0, tk, ti));
    const bool l1 = valid && i1 < N && (identity ? i1 < m_a : erpl_cmp_label(B, i1, tk, ti));
    const u64 b0 = __ballot(l0), b1 = __ballot(l1);
    if (lane == 0) {
      bits[i0 * (u64)wb + word] = b0;
      if (i1 < N) bits[i1 * (u64)wb + word] = b1;
    }
  }
}

// ---- HOT LOOP 1.  grid (ceil(chunks / kWaves), wl); wave -> (chunk, word); no barriers: a wave without a chunk leaves.
struct WalkArgs {
  const uint32_t* sidx;
  const u64* r2e;
  const u64* bits;
  uint32_t* cnt;
  ErplCmpRank* part;
  int64_t N, m_a, len;
  int chunks, wb, wl;
};

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_count(const WalkArgs a) {
  const int lane = threadIdx.x & 63, word = blockIdx.y, c = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (c >= a.chunks) return;
  const int64_t s0 = (int64_t)c * a.len, s1 = s0 + a.len < a.N ? s0 + a.len : a.N;
  uint32_t cnt = 0u;
  for (int64_t base = s0; base < s1; base += 64) {
    const int64_t s = base + lane;
    const u64 mine = s < s1 ? a.bits[(u64)a.sidx[s] * (u64)a.wb + word] : 0ull;
    const int have = (int)(s1 - base < 64 ? s1 - base : 64);
    for (int k = 0; k < have; ++k) cnt += (uint32_t)((word_of_lane(mine, k) >> lane) & 1ull);
  }
  a.cnt[((size_t)c * a.wl + word) * 64 + lane] = cnt;
}

// thread -> a column (word, lane): the counts of the chunks become the number of A members before each chunk
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_scan(uint32_t* __restrict__ cnt, const int chunks, const int cols) {
  const int col = blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x;
  if (col >= cols) return;
  uint32_t run = 0u;
  for (int c = 0; c < chunks; ++c) {
    const uint32_t v = cnt[(size_t)c * cols + col];
    cnt[(size_t)c * cols + col] = run;
    run += v;
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_walk(const WalkArgs a) {
  const int lane = threadIdx.x & 63, word = blockIdx.y, c = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (c >= a.chunks) return;
  const int64_t s0 = (int64_t)c * a.len, s1 = s0 + a.len < a.N ? s0 + a.len : a.N;
  const size_t col = ((size_t)c * a.wl + word) * 64 + lane;
  long long ca = (long long)a.cnt[col];
  long long best = -1, at = 0, sign = 0;
  u64 sum2r = 0ull, sa_lo = 0ull, sa_hi = 0ull, sb_lo = 0ull, sb_hi = 0ull;
  for (int64_t base = s0; base < s1; base += 64) {
    const int64_t s = base + lane;
    const u64 mine = s < s1 ? a.bits[(u64)a.sidx[s] * (u64)a.wb + word] : 0ull;
    const u64 mine_r = s < s1 ? a.r2e[s] : 0ull;
    const int have = (int)(s1 - base < 64 ? s1 - base : 64);
    for (int k = 0; k < have; ++k) {
      const u64 r2e = word_of_lane(mine_r, k), r2 = r2e & ~kEnd;
      const bool on_a = ((word_of_lane(mine, k) >> lane) & 1ull) != 0ull;
      const long long t = base + k + 1;   // members up to and including this position
      ca += on_a ? 1 : 0;
      const long long own = on_a ? ca : t - ca;
      const long long d = (long long)r2 - 2 * own;
      const u64 ad = (u64)(d < 0 ? -d : d);   // <= 2 N < 2^33
      const u64 lo = ad * ad, hi = __umul64hi(ad, ad);
      const u64 a_lo = on_a ? lo : 0ull, a_hi = on_a ? hi : 0ull, b_lo = on_a ? 0ull : lo, b_hi = on_a ? 0ull : hi;
      sa_lo += a_lo; sa_hi += a_hi + (sa_lo < a_lo ? 1ull : 0ull);
      sb_lo += b_lo; sb_hi += b_hi + (sb_lo < b_lo ? 1ull : 0ull);
      sum2r += on_a ? r2 : 0ull;
      if (r2e & kEnd) {   // (uniform) m_b c_A - m_a c_B = N c_A - m_a t: below 2^63 in magnitude
        const long long v = a.N * ca - a.m_a * t, av = v < 0 ? -v : v;
        if (av > best) { best = av; at = base + k; sign = v > 0 ? 1 : (v < 0 ? -1 : 0); }
      }
    }
  }
  ErplCmpRank r;
  r.k = best; r.at = at; r.sign = sign; r.sum2r = sum2r; r.sa_lo = sa_lo; r.sa_hi = sa_hi; r.sb_lo = sb_lo; r.sb_hi = sb_hi;
  a.part[col] = r;
}

// thread -> a column: the chunks in ascending order -> rank[w0 64 + col]; replicate 0 also hands back the value at its `at`
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_rank_fold(const ErplCmpRank* __restrict__ part, const int chunks, const int cols,
                                                                     ErplCmpRank* __restrict__ rank, const int first_col,
                                                                     const uint32_t* __restrict__ sidx, const double* __restrict__ val,
                                                                     double* __restrict__ at_value) {
  const int col = blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x;
  if (col >= cols) return;
  ErplCmpRank r = part[col];
  for (int c = 1; c < chunks; ++c) {
    const ErplCmpRank p = part[(size_t)c * cols + col];
    if (p.k > r.k) { r.k = p.k; r.at = p.at; r.sign = p.sign; }
    r.sum2r += p.sum2r;
    r.sa_lo += p.sa_lo; r.sa_hi += p.sa_hi + (r.sa_lo < p.sa_lo ? 1ull : 0ull);
    r.sb_lo += p.sb_lo; r.sb_hi += p.sb_hi + (r.sb_lo < p.sb_lo ? 1ull : 0ull);
  }
  rank[first_col + col] = r;
  if (first_col + col == 0) *at_value = val[sidx[r.at]];
}

// ---- HOT LOOP 2.  grid (tiles, slices, wl)
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_pairs(const double2* __restrict__ xy, const int64_t N, const int64_t per_slice,
                                                                 const int wb, const u64* __restrict__ bits, double* __restrict__ epart) {
  __shared__ double2 s_z[ERPL_CMP_TILE];
  __shared__ u64 s_w[ERPL_CMP_TILE];
  __shared__ double s_red[kWaves][64][3];
  const int tid = threadIdx.x, word = blockIdx.z;
  const int64_t i = (int64_t)blockIdx.x * ERPL_CMP_TILE + tid;
  const bool have = i < N;
  const double2 zi = have ? xy[i] : make_double2(0.0, 0.0);   // a lane without a member computes and contributes nothing
  const u64 wi = have ? bits[(u64)i * (u64)wb + word] : 0ull;
  const int64_t first = (int64_t)blockIdx.y * per_slice, last = first + per_slice < N ? first + per_slice : N;
  double r[64], t = 0.0;
#pragma unroll
  for (int k = 0; k < 64; ++k) r[k] = 0.0;
  for (int64_t base = first; base < last; base += ERPL_CMP_TILE) {
    const int cnt = (int)(last - base < ERPL_CMP_TILE ? last - base : ERPL_CMP_TILE);
    __syncthreads();   // the stage before has been read
    if (tid < cnt) {
      s_z[tid] = xy[base + tid];
      s_w[tid] = bits[(u64)(base + tid) * (u64)wb + word];
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const double2 z = s_z[j];   // one address per wave: a broadcast
      const u64 w = word_of_lane(s_w[j], 0);   // the same in every lane: into scalar registers
      const uint32_t half[2] = {(uint32_t)w, (uint32_t)(w >> 32)};
      const double dx = zi.x - z.x, dy = zi.y - z.y;
      const double d = sqrt(dx * dx + dy * dy);
      t += d;
#pragma unroll
      for (int k = 0; k < 64; ++k) {
        // 0.0 or 1.0 from two scalar instructions: the sign-extended bit, and the high word of 1.0
        const uint32_t hi = (uint32_t)__builtin_amdgcn_sbfe((int)half[k >> 5], k & 31, 1) & 0x3ff00000u;
        r[k] = __builtin_fma(__hiloint2double((int)hi, 0), d, r[k]);
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const bool on_a = ((wi >> k) & 1ull) != 0ull;
    double aa = have && on_a ? r[k] : 0.0, ab = have && !on_a ? r[k] : 0.0, bb = have && !on_a ? t - r[k] : 0.0;
    wave_fold<Add, Add, Add>(aa, ab, bb);
    if (lane == 0) { s_red[wave][k][0] = aa; s_red[wave][k][1] = ab; s_red[wave][k][2] = bb; }
  }
  __syncthreads();
  if (tid < 192) {
    const int k = tid / 3, which = tid - 3 * k;
    double v = s_red[0][k][which];
    for (int w = 1; w < kWaves; ++w) v += s_red[w][k][which];
    const size_t block = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * gridDim.z + word;
    epart[(block * 64 + k) * 3 + which] = v;
  }
}

// thread -> (column, which): the partial sums in ascending (tile, slice) order
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cmp_pairs_fold(const double* __restrict__ epart, const int blocks, const int cols,
                                                                      double* __restrict__ eout, const int first_col) {
  const int e = blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x;
  if (e >= cols * 3) return;
  double v = epart[e];
  for (int b = 1; b < blocks; ++b) v += epart[(size_t)b * cols * 3 + e];
  eout[(size_t)first_col * 3 + e] = v;
}

}  // namespace

int erpl_launch_cmp_prepare(const ErplCmpArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = (int64_t)a.N;
  const int nb = grid_of(N);
  hipLaunchKernelGGL(erpl_cmp_gather, dim3(nb, a.n_rows + (a.bivariate ? 1 : 0)), dim3(ERPL_ANA_BLOCK), 0, st, a);
  for (int j = 0; j < a.n_rows; ++j) {
    hipLaunchKernelGGL(erpl_cmp_keys, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, N, a.val[j], a.keys, a.idx);
    size_t bytes = a.temp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(a.temp, bytes, a.keys, a.keys + N, a.idx, a.idx + N, (size_t)N, 0, 64, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(erpl_cmp_ranks, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, N, a.keys + N, a.idx + N, a.sidx[j], a.r2e[j]);
  }
  if (a.permutations > 0)
    hipLaunchKernelGGL(erpl_cmp_thresholds, dim3(a.permutations), dim3(ERPL_ANA_BLOCK), 0, st, a.seed, a.N, a.m_a, a.thr);
  return (int)hipGetLastError();
}

int erpl_launch_cmp_block(const ErplCmpArgs& a, int w0, int wl, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = (int64_t)a.N;
  const int Q = a.permutations + 1, cols = wl * 64;
  const u64 pairs = (a.N + 1) / 2;
  const int bits_grid = (int)((pairs + kWaves - 1) / kWaves < ERPL_ANA_MAX_BLOCKS ? (pairs + kWaves - 1) / kWaves : ERPL_ANA_MAX_BLOCKS);
  // the matrix of this block is [N][wl]: rows of exactly the words the block has
  hipLaunchKernelGGL(erpl_cmp_bits, dim3(bits_grid, wl), dim3(ERPL_ANA_BLOCK), 0, st, a.seed, a.N, a.m_a, Q, w0, wl, a.thr, a.bits);
  WalkArgs w;
  w.bits = a.bits; w.cnt = a.cnt; w.part = a.part; w.N = N; w.m_a = (int64_t)a.m_a; w.wb = wl; w.wl = wl;
  w.chunks = erpl_cmp_chunks(N, a.wb, &w.len);
  const dim3 walk_grid((w.chunks + kWaves - 1) / kWaves, wl), col_grid((cols + ERPL_ANA_BLOCK - 1) / ERPL_ANA_BLOCK);
  for (int j = 0; j < a.n_rows; ++j) {
    w.sidx = a.sidx[j]; w.r2e = a.r2e[j];
    hipLaunchKernelGGL(erpl_cmp_count, walk_grid, dim3(ERPL_ANA_BLOCK), 0, st, w);
    hipLaunchKernelGGL(erpl_cmp_scan, col_grid, dim3(ERPL_ANA_BLOCK), 0, st, a.cnt, w.chunks, cols);
    hipLaunchKernelGGL(erpl_cmp_walk, walk_grid, dim3(ERPL_ANA_BLOCK), 0, st, w);
    hipLaunchKernelGGL(erpl_cmp_rank_fold, col_grid, dim3(ERPL_ANA_BLOCK), 0, st, a.part, w.chunks, cols,
                       a.rank + (size_t)j * a.words * 64, w0 * 64, a.sidx[j], a.val[j], a.at_value + j);
  }
  if (a.bivariate) {
    int64_t per_slice;
    const int slices = erpl_cmp_slices(N, a.wb, &per_slice);
    const int tiles = (int)((N + ERPL_CMP_TILE - 1) / ERPL_CMP_TILE);
    hipLaunchKernelGGL(erpl_cmp_pairs, dim3(tiles, slices, wl), dim3(ERPL_ANA_BLOCK), 0, st, reinterpret_cast<const double2*>(a.xy), N,
                       per_slice, wl, a.bits, a.epart);
    hipLaunchKernelGGL(erpl_cmp_pairs_fold, dim3((cols * 3 + ERPL_ANA_BLOCK - 1) / ERPL_ANA_BLOCK), dim3(ERPL_ANA_BLOCK), 0, st, a.epart,
                       tiles * slices, cols, a.eout, w0 * 64);
  }
  return (int)hipGetLastError();
}
