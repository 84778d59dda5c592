// erpl_corridor_drivers.hip — erpl_mc_corridor_drivers and its defaults of the C ABI (include/erpl_mc.h): for every row of a
// time-resolved matrix and every per-sample factor the correlation and the standardised regression coefficient over the row's
// own population.  The host rules (sums -> pearson / src / r2 / ok) are erpl_cdrv.h, the buffer is laid out in
// erpl_stat_layout.h.
//
//   base      one pass over the F factor rows: a byte per column (0 = mask byte 0 and every factor finite, 1 = masked, 2 = a
//             factor that is not finite) and the three counts (ballots, 64-bit integer atomics)
//   moments   workgroup (segment, row) over a matrix [rows][ld] - the factors, then the values: count, sum, min, max of the
//             finite values in base columns, then the centred squares; a thread takes its columns in index order, the
//             workgroup folds in the fixed order of erpl_stat_device.h, one thread per row folds the segments in order
//   product   the hot pass.  Workgroup (tile of 32 rows, slice of m), four waves.  A stage of 16 members goes through LDS:
//             the left operand [member][64] - the memberships m_r of the 32 rows, then m_r y'_r - and the standardised
//             factors [member][48] (x'_f, the ones at 32, zeros behind them); standardisation and masking happen on the way
//             in, the next stage is on its way from global memory into registers meanwhile.  Per 4 members a wave issues
//             v_mfma_f64_16x16x4_f64 on 16 x 16 blocks: waves 0 .. 2 own a block of 16 linear columns each, for the
//             memberships (sum m x'_f, the count) and for the y' rows (sum m y' x'_f, sum m y'); every wave owns the product
//             blocks b = wave, wave + 4, .. for the memberships, whose right operand x'_f x'_g is one multiply of two LDS
//             reads (ERPL_CDRV_MFMA = 0: the same blocks, stages and partial sums on v_fma_f64, the measured baseline).
//             sum m y'^2 is added up by the threads that stage y' and folded through LDS in member order.  The record of a
//             (tile, slice) is written once.
//   fold      sums[row][.] = (slice 0 + slice 1) + ..: in slice order.
//   extremes  one workgroup per (row, factor) whose sums leave open whether the factor is constant over the row's population:
//             its exact min / max there.
// Segments and slices are functions of m alone, a tile's arithmetic does not depend on the other tiles, and every
// floating-point sum has a fixed order: the same bits in every call, and for a row whatever other rows are in the call.  No
// floating-point atomics, every loop bounded.  Compiled with -ffp-contract=off like its siblings; the fused multiply-adds of
// the product pass are written out.
#include <string.h>

#include <algorithm>
#include <vector>

#include "erpl_cdrv.h"
#include "erpl_host.h"
#include "erpl_stat_device.h"

namespace {

// 1: the product pass on v_mfma_f64_16x16x4_f64; 0: on v_fma_f64, the baseline it is measured against
#ifndef ERPL_CDRV_MFMA
#define ERPL_CDRV_MFMA 1
#endif
typedef double double4v __attribute__((ext_vector_type(4)));

constexpr int kTR = ERPL_CDRV_TILE_ROWS, kKT = ERPL_CDRV_KT, kLin = ERPL_CDRV_LIN;
constexpr int kLdl = 2 * kTR + 2, kLdx = kLin + 2;
constexpr int kStat = 8;   // doubles of a moment record: count (its 64 bits), mean, std, min, max, 1 / std or 0, two spare
static_assert(kTR == 32 && kKT == 16 && ERPL_ANA_BLOCK == 256, "four waves: 16 members x 16 rows per staging step");

// ---- base: the byte of every column and the three counts
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cdrv_base(const double* __restrict__ factors, const int64_t ldf, const int F,
                                                                  const uint8_t* __restrict__ mask, const int64_t m,
                                                                  uint8_t* __restrict__ base, u64* __restrict__ counter) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  u64 cnt[3] = {0ull, 0ull, 0ull};   // base, masked, factor not finite: uniform over the wave
  for (int64_t first = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + wave * 64; first < m; first += stride) {
    const int64_t i = first + lane;
    int why = -1;
    if (i < m) {
      why = (mask && mask[i] != 0) ? 1 : 0;
      if (why == 0)
        for (int f = 0; f < F; ++f)
          if (!finite_bits(factors[(int64_t)f * ldf + i])) why = 2;
      base[i] = (uint8_t)why;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) cnt[k] += __popcll(__ballot(why == k));
  }
  const u64 s = counters_fold(cnt);
  if (threadIdx.x < 3 && s) atomicAdd(&counter[threadIdx.x], s);
}

// ---- moments of row blockIdx.y of X over segment blockIdx.x: the finite values in base columns
template <int PASS>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cdrv_moments(const double* __restrict__ X, const int64_t ld,
                                                                     const uint8_t* __restrict__ base, const int64_t m,
                                                                     const int64_t seg_len, const double* __restrict__ stat,
                                                                     double* __restrict__ part) {
  const int row = blockIdx.y;
  const double* __restrict__ x = X + (int64_t)row * ld;
  const int64_t begin = (int64_t)blockIdx.x * seg_len;
  const int64_t end = begin + seg_len < m ? begin + seg_len : m;
  double* __restrict__ p = part + ((size_t)row * gridDim.x + blockIdx.x) * 4;
  if (PASS == 0) {
    u64 cnt = 0ull;
    double sum = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t i = begin + threadIdx.x; i < end; i += ERPL_ANA_BLOCK) {
      if (base[i] != 0) continue;
      const double v = x[i];
      if (!finite_bits(v)) continue;
      ++cnt;
      sum += v;
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
    }
    block_fold<Add, Add, Min, Max>(cnt, sum, mn, mx);
    if (threadIdx.x == 0) { p[0] = from_bits<double>(cnt); p[1] = sum; p[2] = mn; p[3] = mx; }
  } else {
    const double mean = stat[(size_t)row * kStat + 1];
    double ss = 0.0;
    for (int64_t i = begin + threadIdx.x; i < end; i += ERPL_ANA_BLOCK) {
      if (base[i] != 0) continue;
      const double v = x[i];
      if (!finite_bits(v)) continue;
      const double d = v - mean;
      ss += d * d;
    }
    block_fold<Add>(ss);
    if (threadIdx.x == 0) p[0] = ss;
  }
}
// one thread per row: the segments in order
template <int PASS>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cdrv_finish(const double* __restrict__ part, const int segs, const int rows,
                                                                    double* __restrict__ stat) {
  const int row = blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x;
  if (row >= rows) return;
  const double* __restrict__ p = part + (size_t)row * segs * 4;
  double* __restrict__ o = stat + (size_t)row * kStat;
  if (PASS == 0) {
    u64 cnt = 0ull;
    double sum = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int s = 0; s < segs; ++s) {
      cnt += bits_of(p[4 * s]);
      sum += p[4 * s + 1];
      mn = p[4 * s + 2] < mn ? p[4 * s + 2] : mn;
      mx = p[4 * s + 3] > mx ? p[4 * s + 3] : mx;
    }
    o[0] = from_bits<double>(cnt);
    o[1] = sum / (double)cnt;   // NaN for an empty population
    o[2] = NAN; o[3] = mn; o[4] = mx; o[5] = 0.0; o[6] = 0.0; o[7] = 0.0;
  } else {
    double ss = 0.0;
    for (int s = 0; s < segs; ++s) ss += p[4 * s];
    const double sd = sqrt(ss / (double)bits_of(o[0]));
    o[2] = sd;
    o[5] = (sd > 0.0 && finite_bits(sd)) ? 1.0 / sd : 0.0;   // a constant row or factor is standardised to zeros
  }
}

// ---- product: workgroup (tile, slice) -> part[slice][tile][32][rd]
// NPB: product blocks a wave owns at the most (9 with the regression: 33 blocks of 16 over four waves; 1 without)
template <int NPB>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cdrv_product(const double* __restrict__ factors, const int64_t ldf, const int F,
                                                                     const double* __restrict__ values, const int64_t ld, const int rows,
                                                                     const int row0, const uint8_t* __restrict__ base, const int64_t m,
                                                                     const int64_t slice_len, const double* __restrict__ fstat,
                                                                     const double* __restrict__ rstat, const int npb, const int P,
                                                                     const int rd, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double s_l[kKT][kLdl];   // [member][m_r of the 32 rows, then m_r y'_r]
  __shared__ __attribute__((aligned(16))) double s_x[kKT][kLdx];   // [member][x'_f, the ones, zeros]
  static_assert(kKT * kLdl >= kTR * 16, "the fold of sum y'^2 reuses the left operand");
  const int tid = threadIdx.x, lk = tid & 15, li = tid >> 4;   // staging: member lk of the stage, rows / factors li and li + 16
  const int wave = tid >> 6, lane = tid & 63, c = lane & 15, kq = lane >> 4;
  const int64_t k_begin = (int64_t)blockIdx.y * slice_len;
  const int64_t k_end = k_begin + slice_len < m ? k_begin + slice_len : m;

  const double* py[2];
  const double* px[2];
  bool in_row[2], in_f[2];
  double rmean[2], rinv[2], xmean[2], xinv[2], syy[2] = {0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int row = row0 + blockIdx.x * kTR + li + 16 * r, f = li + 16 * r;
    in_row[r] = row < rows; in_f[r] = f < F;
    py[r] = values + (int64_t)(in_row[r] ? row : 0) * ld;   // a row past the matrix is never read
    px[r] = factors + (int64_t)(in_f[r] ? f : 0) * ldf;
    rmean[r] = in_row[r] ? rstat[(size_t)row * kStat + 1] : 0.0;
    rinv[r] = in_row[r] ? rstat[(size_t)row * kStat + 5] : 0.0;
    xmean[r] = in_f[r] ? fstat[(size_t)f * kStat + 1] : 0.0;
    xinv[r] = in_f[r] ? fstat[(size_t)f * kStat + 5] : 0.0;
  }
  for (int e = tid; e < kKT * kLdx; e += ERPL_ANA_BLOCK) (&s_x[0][0])[e] = (e % kLdx) == ERPL_CDRV_ONE ? 1.0 : 0.0;
  __syncthreads();   // the stages write the factor columns of the same lines

  // the columns of the product blocks this lane feeds: x'_f x'_g at column c of block wave + 4 j (zeros past the last product)
  int off_f[NPB], off_g[NPB];
#pragma unroll
  for (int j = 0; j < NPB; ++j) {
    const int p = (wave + 4 * j) * 16 + c;
    int f = ERPL_CDRV_ZERO, g = ERPL_CDRV_ZERO;
    if (wave + 4 * j < npb && p < P) {
      if (p < F) {
        f = g = p;
      } else {
        int q = p - F;
        f = 0;
        while (f < F - 1 && q >= F - 1 - f) { q -= F - 1 - f; ++f; }
        g = f + 1 + q;
      }
    }
    off_f[j] = f; off_g[j] = g;
  }
  const bool lin_on = wave == 2 || (wave < 2 && wave * 16 < F);   // block 2 holds the ones

  double4v accp[NPB][2], accl[4];
#pragma unroll
  for (int j = 0; j < NPB; ++j) accp[j][0] = accp[j][1] = double4v{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) accl[j] = double4v{0.0, 0.0, 0.0, 0.0};

  double ry[2], rx[2];
  int rb = 1;
  auto load = [&](int64_t k0) {
    const int64_t k = k0 + lk;
    const bool in_k = k < k_end;   // k_end <= m <= ld, ldf
    rb = in_k ? (int)base[k] : 1;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      ry[r] = in_k && in_row[r] ? py[r][k] : (double)NAN;
      rx[r] = in_k && in_f[r] ? px[r][k] : 0.0;
    }
  };
  if (k_begin < k_end) load(k_begin);
  for (int64_t k0 = k_begin; k0 < k_end; k0 += kKT) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const bool mem = rb == 0 && in_row[r] && finite_bits(ry[r]);
      const double yv = mem ? (ry[r] - rmean[r]) * rinv[r] : 0.0;
      s_l[lk][li + 16 * r] = mem ? 1.0 : 0.0;
      s_l[lk][kTR + li + 16 * r] = yv;
      syy[r] = __builtin_fma(yv, yv, syy[r]);
      s_x[lk][li + 16 * r] = (rb == 0 && in_f[r]) ? (rx[r] - xmean[r]) * xinv[r] : 0.0;
    }
    __syncthreads();
    if (k0 + kKT < k_end) load(k0 + kKT);
#if ERPL_CDRV_MFMA
    // per 4 members one v_mfma_f64_16x16x4_f64 per block: lane l hands in row (l & 15) of the left block and column (l & 15)
    // of the right one at member (l >> 4)
#pragma unroll
    for (int kg = 0; kg < kKT / 4; ++kg) {
      const int k = kg * 4 + kq;
      const double am0 = s_l[k][c], am1 = s_l[k][16 + c];
      if (lin_on) {
        const double ay0 = s_l[k][kTR + c], ay1 = s_l[k][kTR + 16 + c], bl = s_x[k][wave * 16 + c];
        accl[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(am0, bl, accl[0], 0, 0, 0);
        accl[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(am1, bl, accl[1], 0, 0, 0);
        accl[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay0, bl, accl[2], 0, 0, 0);
        accl[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay1, bl, accl[3], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < NPB; ++j) {
        if (wave + 4 * j >= npb) continue;
        const double b = s_x[k][off_f[j]] * s_x[k][off_g[j]];
        accp[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(am0, b, accp[j][0], 0, 0, 0);
        accp[j][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(am1, b, accp[j][1], 0, 0, 0);
      }
    }
#else
    // the same blocks on v_fma_f64: lane l keeps rows (l >> 4) + 4 r, column (l & 15) of a block and adds its members in order
#pragma unroll
    for (int k = 0; k < kKT; ++k) {
      double am[2][4], ay[2][4];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          am[b][r] = s_l[k][b * 16 + kq + 4 * r];
          ay[b][r] = lin_on ? s_l[k][kTR + b * 16 + kq + 4 * r] : 0.0;
        }
      if (lin_on) {
        const double bl = s_x[k][wave * 16 + c];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            accl[b][r] = __builtin_fma(am[b][r], bl, accl[b][r]);
            accl[2 + b][r] = __builtin_fma(ay[b][r], bl, accl[2 + b][r]);
          }
      }
#pragma unroll
      for (int j = 0; j < NPB; ++j) {
        if (wave + 4 * j >= npb) continue;
        const double bp = s_x[k][off_f[j]] * s_x[k][off_g[j]];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) accp[j][b][r] = __builtin_fma(am[b][r], bp, accp[j][b][r]);
      }
    }
#endif
    __syncthreads();
  }

  // result r of a block in lane l: row (l >> 4) + 4 r, column l & 15 of the block
  double* __restrict__ out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(kTR * rd);
  const int ycol = kLin + 16 * npb;
  if (wave < 3) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        out[(size_t)(b * 16 + kq + 4 * r) * rd + wave * 16 + c] = accl[b][r];
        out[(size_t)(b * 16 + kq + 4 * r) * rd + ycol + wave * 16 + c] = accl[2 + b][r];
      }
  }
#pragma unroll
  for (int j = 0; j < NPB; ++j) {
    if (wave + 4 * j >= npb) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(b * 16 + kq + 4 * r) * rd + kLin + (wave + 4 * j) * 16 + c] = accp[j][b][r];
  }
  // sum m y'^2 of row li + 16 r: the 16 staging threads of the row, in member order (the loop above ends on a barrier)
  double* red = &s_l[0][0];
#pragma unroll
  for (int r = 0; r < 2; ++r) red[(li + 16 * r) * 16 + lk] = syy[r];
  __syncthreads();
  if (tid < kTR) {
    double s = 0.0;
    for (int k = 0; k < 16; ++k) s += red[tid * 16 + k];
    out[(size_t)tid * rd + ycol + kLin] = s;
    for (int k = ycol + kLin + 1; k < rd; ++k) out[(size_t)tid * rd + k] = 0.0;
  }
}

// ---- fold: the records of a tile in slice order
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cdrv_fold(const double* __restrict__ part, const int slices, const int len,
                                                                  double* __restrict__ sums) {
  const int el = blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x;   // < kTR rd
  if (el >= len) return;
  const size_t step = (size_t)gridDim.y * (size_t)len;
  const double* __restrict__ p = part + (size_t)blockIdx.y * (size_t)len + el;
  double acc = 0.0;
  for (int s = 0; s < slices; ++s) acc += p[(size_t)s * step];
  sums[(size_t)blockIdx.y * (size_t)len + el] = acc;
}

// ---- extremes: min / max of factor pairs[2 j + 1] over the population of row pairs[2 j]
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_cdrv_extremes(const double* __restrict__ factors, const int64_t ldf,
                                                                      const double* __restrict__ values, const int64_t ld,
                                                                      const uint8_t* __restrict__ base, const int64_t m,
                                                                      const int32_t* __restrict__ pairs, double* __restrict__ ext) {
  const double* __restrict__ y = values + (int64_t)pairs[2 * blockIdx.x] * ld;
  const double* __restrict__ x = factors + (int64_t)pairs[2 * blockIdx.x + 1] * ldf;
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t i = threadIdx.x; i < m; i += ERPL_ANA_BLOCK) {
    if (base[i] != 0 || !finite_bits(y[i])) continue;
    const double v = x[i];
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  block_fold<Min, Max>(mn, mx);
  if (threadIdx.x == 0) { ext[2 * blockIdx.x] = mn; ext[2 * blockIdx.x + 1] = mx; }
}

// count, mean, std, min, max of a matrix [rows][ld] into stat[rows][kStat]
void cdrv_launch_moments(const double* X, int64_t ld, int rows, const uint8_t* base, int64_t m, const ErplCdrvLayout& at, double* stat,
                         double* mpart, hipStream_t st) {
  const dim3 grid((unsigned)at.segs, (unsigned)rows), fin((unsigned)((rows + ERPL_ANA_BLOCK - 1) / ERPL_ANA_BLOCK));
  hipLaunchKernelGGL(erpl_cdrv_moments<0>, grid, dim3(ERPL_ANA_BLOCK), 0, st, X, ld, base, m, at.seg_len, (const double*)stat, mpart);
  hipLaunchKernelGGL(erpl_cdrv_finish<0>, fin, dim3(ERPL_ANA_BLOCK), 0, st, (const double*)mpart, at.segs, rows, stat);
  hipLaunchKernelGGL(erpl_cdrv_moments<1>, grid, dim3(ERPL_ANA_BLOCK), 0, st, X, ld, base, m, at.seg_len, (const double*)stat, mpart);
  hipLaunchKernelGGL(erpl_cdrv_finish<1>, fin, dim3(ERPL_ANA_BLOCK), 0, st, (const double*)mpart, at.segs, rows, stat);
}

u64 stat_count(const double* rec) {
  u64 b;
  memcpy(&b, rec, sizeof(b));
  return b;
}

}  // namespace

extern "C" {

int erpl_mc_corridor_drivers_defaults(erpl_cdrv_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  memset(spec, 0, sizeof(*spec));
  spec->regression = 1;
  return ERPL_OK;
}

int erpl_mc_corridor_drivers(erpl_ctx* c, const double* factors, int64_t ldf, const double* values, int64_t ld, const uint8_t* mask,
                             int64_t m, const erpl_cdrv_spec* spec, erpl_cdrv_result* result, erpl_cdrv_row* rows, double* pearson,
                             double* src, void* stream) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (!factors) return erpl_fail(ERPL_ERR_INVALID, "factors is NULL");
  if (!values) return erpl_fail(ERPL_ERR_INVALID, "values is NULL");
  if (!result) return erpl_fail(ERPL_ERR_INVALID, "result is NULL");
  if (!rows) return erpl_fail(ERPL_ERR_INVALID, "rows is NULL");
  if (!pearson) return erpl_fail(ERPL_ERR_INVALID, "pearson is NULL");
  if (m <= 0 || m > 2147483647LL) return erpl_fail(ERPL_ERR_INVALID, "m = %lld outside 1..2^31 - 1", (long long)m);
  if (ld < m) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below m = %lld", (long long)ld, (long long)m);
  if (ldf < m) return erpl_fail(ERPL_ERR_INVALID, "ldf = %lld is below m = %lld", (long long)ldf, (long long)m);
  if (spec->n_factors < 1 || spec->n_factors > ERPL_CDRV_MAX_FACTORS)
    return erpl_fail(ERPL_ERR_INVALID, "spec->n_factors = %d outside 1..%d", spec->n_factors, ERPL_CDRV_MAX_FACTORS);
  if (spec->n_rows < 1 || spec->n_rows > ERPL_CDRV_MAX_ROWS)
    return erpl_fail(ERPL_ERR_INVALID, "spec->n_rows = %d outside 1..%d", spec->n_rows, ERPL_CDRV_MAX_ROWS);
  if (spec->regression != 0 && spec->regression != 1)
    return erpl_fail(ERPL_ERR_INVALID, "spec->regression = %d: 0 or 1", spec->regression);
  if (!spec->regression && src) return erpl_fail(ERPL_ERR_INVALID, "src is given but spec->regression = 0");
  if (spec->regression && !src) return erpl_fail(ERPL_ERR_INVALID, "src is NULL but spec->regression = 1");
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int F = spec->n_factors, R = spec->n_rows;
  const bool reg = spec->regression != 0;
  const double nan = NAN;

  const ErplCdrvLayout at = erpl_cdrv_layout(m, R, F, reg);
  ERPL_TRY(c->cdrv.grow(at.need));
  char* buf = c->cdrv.buf;
  uint8_t* base = (uint8_t*)(buf + at.base);
  u64* counter = (u64*)(buf + at.count);
  double* fstat = (double*)(buf + at.fstat);
  double* rstat = (double*)(buf + at.rstat);
  double* mpart = (double*)(buf + at.mpart);

  // pass 0: the base bytes and the factors over P0; pass 1: the rows over their own populations
  HIP_TRY(hipMemsetAsync(counter, 0, 32, st));
  hipLaunchKernelGGL(erpl_cdrv_base, dim3(grid_of(m)), dim3(ERPL_ANA_BLOCK), 0, st, factors, ldf, F, mask, m, base, counter);
  cdrv_launch_moments(factors, ldf, F, base, m, at, fstat, mpart, st);
  cdrv_launch_moments(values, ld, R, base, m, at, rstat, mpart, st);
  HIP_TRY(hipGetLastError());
  u64 h_count[4];
  std::vector<double> h_fstat((size_t)F * kStat), h_rstat((size_t)R * kStat);
  HIP_TRY(hipMemcpyAsync(h_count, counter, sizeof(h_count), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_fstat.data(), fstat, h_fstat.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_rstat.data(), rstat, h_rstat.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  memset(result, 0, sizeof(*result));
  result->m = m;
  result->n_base = (int64_t)h_count[0];
  result->n_masked = (int64_t)h_count[1];
  result->n_factor_non_finite = (int64_t)h_count[2];
  const bool any = h_count[0] > 0ull;
  for (int f = 0; f < ERPL_CDRV_MAX_FACTORS; ++f) {
    const bool in = any && f < F;
    const double* s = h_fstat.data() + (size_t)(in ? f : 0) * kStat;
    result->mean[f] = in ? s[1] : nan; result->std[f] = in ? s[2] : nan;
    result->min[f] = in ? s[3] : nan; result->max[f] = in ? s[4] : nan;
    result->constant[f] = in && s[3] == s[4] ? 1 : 0;
  }
  for (int r = 0; r < R; ++r) {
    const double* s = h_rstat.data() + (size_t)r * kStat;
    erpl_cdrv_row& o = rows[r];
    memset(&o, 0, sizeof(o));
    o.count = (int64_t)stat_count(s);
    const bool in = o.count > 0;
    o.mean = in ? s[1] : nan; o.std = in ? s[2] : nan; o.min = in ? s[3] : nan; o.max = in ? s[4] : nan;
    o.constant = in && s[3] == s[4] ? 1 : 0;
    o.r2 = o.pivot_min = nan;
  }

  // the product pass, a chunk of tiles at a time
  const int rd = at.row_doubles, npb = erpl_cdrv_product_blocks(F, reg), P = erpl_cdrv_products(F, reg);
  const int tiles = (R + kTR - 1) / kTR, tile_len = kTR * rd;
  double* part = (double*)(buf + at.part);
  double* sums = (double*)(buf + at.sums);
  int32_t* d_pairs = (int32_t*)(buf + at.pairs);
  double* d_ext = (double*)(buf + at.ext);
  std::vector<double> h_sums, h_ext;
  std::vector<int32_t> h_pairs, fconst;
  for (int t0 = 0; t0 < tiles; t0 += at.chunk_tiles) {
    const int nt = std::min(at.chunk_tiles, tiles - t0), row0 = t0 * kTR, nrows = std::min(nt * kTR, R - row0);
    const dim3 grid((unsigned)nt, (unsigned)at.slices);
    if (reg)
      hipLaunchKernelGGL(erpl_cdrv_product<9>, grid, dim3(ERPL_ANA_BLOCK), 0, st, factors, ldf, F, values, ld, R, row0, (const uint8_t*)base,
                         m, at.slice_len, (const double*)fstat, (const double*)rstat, npb, P, rd, part);
    else
      hipLaunchKernelGGL(erpl_cdrv_product<1>, grid, dim3(ERPL_ANA_BLOCK), 0, st, factors, ldf, F, values, ld, R, row0, (const uint8_t*)base,
                         m, at.slice_len, (const double*)fstat, (const double*)rstat, npb, P, rd, part);
    hipLaunchKernelGGL(erpl_cdrv_fold, dim3((unsigned)((tile_len + ERPL_ANA_BLOCK - 1) / ERPL_ANA_BLOCK), (unsigned)nt), dim3(ERPL_ANA_BLOCK),
                       0, st, (const double*)part, at.slices, tile_len, sums);
    HIP_TRY(hipGetLastError());
    h_sums.resize((size_t)nt * tile_len);
    HIP_TRY(hipMemcpyAsync(h_sums.data(), sums, h_sums.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    // which factors are constant over which row's population: proven not to be by the sums, or by their exact extremes
    fconst.assign((size_t)nrows * F, 0);
    h_pairs.clear();
    for (int j = 0; j < nrows; ++j) {
      const int64_t count = rows[row0 + j].count;
      if (count < 2) continue;   // everything of such a row is NaN already
      const ErplCdrvRowView v = erpl_cdrv_row_view(h_sums.data() + (size_t)j * rd, F, reg);
      for (int f = 0; f < F; ++f) {
        if (result->constant[f]) { fconst[(size_t)j * F + f] = 1; continue; }
        if (erpl_cdrv_ambiguous(v.c[f], v.a[f], (double)count)) { h_pairs.push_back(row0 + j); h_pairs.push_back(f); }
      }
    }
    if (!h_pairs.empty()) {
      const size_t np = h_pairs.size() / 2;
      h_ext.resize(2 * np);
      HIP_TRY(hipMemcpyAsync(d_pairs, h_pairs.data(), h_pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(erpl_cdrv_extremes, dim3((unsigned)np), dim3(ERPL_ANA_BLOCK), 0, st, factors, ldf, values, ld, (const uint8_t*)base,
                         m, (const int32_t*)d_pairs, d_ext);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(h_ext.data(), d_ext, h_ext.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (size_t k = 0; k < np; ++k)
        if (h_ext[2 * k] == h_ext[2 * k + 1]) fconst[(size_t)(h_pairs[2 * k] - row0) * F + h_pairs[2 * k + 1]] = 1;
    }
    for (int j = 0; j < nrows; ++j) {
      erpl_cdrv_row& o = rows[row0 + j];
      const ErplCdrvRowView v = erpl_cdrv_row_view(h_sums.data() + (size_t)j * rd, F, reg);
      erpl_cdrv_finish_row(F, reg, o.count, o.constant != 0, fconst.data() + (size_t)j * F, v, pearson + (size_t)(row0 + j) * F,
                           reg ? src + (size_t)(row0 + j) * F : nullptr, &o.r2, &o.pivot_min, &o.regression_ok);
    }
  }
  return ERPL_OK;
}

}  // extern "C"
