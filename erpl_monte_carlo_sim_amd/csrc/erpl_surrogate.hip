// erpl_surrogate.hip — erpl_mc_surrogate, erpl_mc_surrogate_predict, _predict_host, _terms and _defaults of the C ABI
// (include/erpl_mc.h): a polynomial chaos surrogate of a run of independent primitives.  The basis, the terms and the
// evaluation of the polynomial are those of erpl_pce.h, here for the device and for the host.  The population bytes come
// from the first pass of erpl_correlation.hip and are compacted by the select of erpl_bootstrap.hip; what is here works on
// the dense population of m members, of which the fitted ones (all, or all but every k-th) are numbered e = 0 .. n_fit - 1.
//
//   basis     a workgroup of T = erpl_sur_group samples, one thread each: the univariate values of the sample into LDS
//             (u[(v degree + k - 1) T + thread]: no bank conflicts), then every term as the product of its factors and the
//             requested outcomes behind them: A[cols][ld], cols = P + R, a row per term, members contiguous.
//   gram      the hot pass: A A^T of a chunk.  One workgroup per (pair of 128 x 128 tiles of the upper triangle, slice of
//             the chunk): four waves with a 64 x 64 quarter each, 4 x 4 blocks of v_mfma_f64_16x16x4_f64 (ERPL_SUR_MFMA = 0:
//             256 threads with 8 x 8 results each on v_fma_f64, the measured baseline); the two operand panels go through
//             LDS 16 members at a time ([member][row + 2]), the next stage is on its way from global memory into registers
//             meanwhile; every result adds its products in ascending member order, fused.  The partial tile of a (pair,
//             slice) is written once.
//   fold      gram[i][j] = ((gram[i][j] + slice 0) + slice 1) + ..: in slice order, chunk after chunk.
//   predict   the basis kernel's first half, then acc = c_0, acc = acc + (c_t Psi_t) for every requested row.  Also the
//             fitted values of the members (through `src`) for the residual passes.
//   sums      two streaming passes in the fixed order of erpl_stat_device.h: the sums of y over the fitted and the held-out
//             members, then the centred squares and the squared residuals.
// The slices are functions of (n_fit, P) alone (erpl_sur_slices), the tiles and grids of (n_fit, P, n_rows), and every
// floating-point sum has a fixed order that the slices decide: the same bits in every call, and for a row whatever other rows
// are requested with it.  No floating-point atomics.  Compiled with -ffp-contract=off like its siblings, so that predict carries
// the bits of erpl_mc_surrogate_predict_host; the fused multiply-adds of the Gram kernel are written out.
#include <string.h>

#include <algorithm>
#include <vector>

#include "erpl_host.h"
#include "erpl_pce.h"
#include "erpl_stat_device.h"

namespace {

// 1: the Gram kernel on v_mfma_f64_16x16x4_f64; 0: on v_fma_f64, the baseline it was measured against (the same tiles,
// stages and partial sums; 45.5 against 33.0 TFLOP/s at n_fit = 1 048 576, P = 976: DESIGN.md section 8.13)
#ifndef ERPL_SUR_MFMA
#define ERPL_SUR_MFMA 1
#endif
typedef double double4v __attribute__((ext_vector_type(4)));

constexpr int kTile = ERPL_SUR_TILE, kKT = ERPL_SUR_KT, kRB = kTile / 16, kLdt = kTile + 2;
constexpr int kTermBytes = 2 * ERPL_PCE_SLOTS;

// the model as the kernels read it: pieces of the model buffer (erpl_sur_model_pieces)
struct ErplSurModel {
  const ErplPceTables* tab;
  const uint8_t* kinds;
  const int8_t* terms;      // [P][4][2]
  const double* coef;       // [n_rows][P]
  int32_t n_vars, n_rows, degree, n_terms;
};

// the fitted member e is the dense member e (no holdout) or the e-th one that is not a multiple of k away from k - 1
__host__ __device__ inline int64_t sur_fit_member(int64_t e, int k) { return k ? e + e / (k - 1) : e; }
__device__ __forceinline__ bool sur_held_out(int64_t d, int k) { return k && d % k == k - 1; }

// the univariate values of thread's sample into u[.. * T + thread]; false: an input is not finite
__device__ __forceinline__ bool sur_univariate(const ErplSurModel& M, const double* __restrict__ x, int64_t ldx, int64_t col, double* u,
                                               int T) {
  bool ok = true;
  for (int v = 0; v < M.n_vars; ++v) {
    const double xv = x[(int64_t)v * ldx + col];
    ok = ok && erpl_pce_finite(xv);
    erpl_pce_univariate(*M.tab, M.kinds[v], xv, M.degree, u + (size_t)v * M.degree * T, T);
  }
  return ok;
}

// ---- basis: members e0 .. e0 + len - 1 of the fitted ones -> A[cols][ld]
struct ErplSurRows {
  const double* y[ERPL_SUR_MAX_ROWS];   // [n] each: the requested rows
};
__global__ void erpl_sur_basis(const ErplSurModel M, const double* __restrict__ x, const ErplSurRows yrow, int64_t n,
                               const uint32_t* __restrict__ src, int holdout, int64_t e0, int len, double* __restrict__ A, int64_t ld) {
  extern __shared__ double s_u[];
  const int T = blockDim.x, e = blockIdx.x * T + threadIdx.x;
  if (e >= len) return;
  const int64_t col = src[sur_fit_member(e0 + e, holdout)];
  double* u = s_u + threadIdx.x;
  sur_univariate(M, x, n, col, u, T);
  for (int t = 0; t < M.n_terms; ++t) A[(int64_t)t * ld + e] = erpl_pce_term(M.terms + (size_t)t * kTermBytes, u, M.degree, T);
  for (int j = 0; j < M.n_rows; ++j) A[(int64_t)(M.n_terms + j) * ld + e] = yrow.y[j][col];
}

// ---- gram: workgroup (pair, slice).  part[slice][pair][kTile][kTile].
__global__ __launch_bounds__(256) void erpl_sur_gram(const double* __restrict__ A, const int64_t ld, const int cols, const int len,
                                                     const int slice_len, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double s_a[kKT][kLdt];
  __shared__ __attribute__((aligned(16))) double s_b[kKT][kLdt];
  // pair -> (ti, tj), ti <= tj: the pairs of row ti start at ti tiles - ti (ti - 1) / 2
  const int tiles = (cols + kTile - 1) / kTile;
  int ti = 0, left = blockIdx.x;
  while (left >= tiles - ti) { left -= tiles - ti; ++ti; }
  const int tj = ti + left;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;   // results: rows ty kRB + i, columns tx kRB + j
  const int lk = tid & 15, li = tid >> 4;                      // loads: member lk of the stage, rows li + 16 r
  const int k_begin = blockIdx.y * slice_len;
  const int k_end = k_begin + slice_len < len ? k_begin + slice_len : len;

#if ERPL_SUR_MFMA
  static_assert(kTile == 128, "four waves, a 64 x 64 quarter each");
  (void)tx; (void)ty;
  double4v macc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) macc[i][j] = double4v{0.0, 0.0, 0.0, 0.0};
#else
  double acc[kRB][kRB];
#pragma unroll
  for (int i = 0; i < kRB; ++i)
#pragma unroll
    for (int j = 0; j < kRB; ++j) acc[i][j] = 0.0;
#endif
  double ra[kRB], rb[kRB];
  const double* pa[kRB];
  const double* pb[kRB];
  bool in_a[kRB], in_b[kRB];
#pragma unroll
  for (int r = 0; r < kRB; ++r) {
    const int row_a = ti * kTile + li + 16 * r, row_b = tj * kTile + li + 16 * r;
    in_a[r] = row_a < cols; in_b[r] = row_b < cols;
    pa[r] = A + (int64_t)(in_a[r] ? row_a : 0) * ld;   // a row past the matrix is never read: it loads zeros
    pb[r] = A + (int64_t)(in_b[r] ? row_b : 0) * ld;
  }
  auto load = [&](int k0) {
    const int k = k0 + lk;
    const bool in_k = k < k_end;   // k_end <= len <= ld
#pragma unroll
    for (int r = 0; r < kRB; ++r) {
      ra[r] = in_k && in_a[r] ? pa[r][k] : 0.0;
      rb[r] = in_k && in_b[r] ? pb[r][k] : 0.0;
    }
  };
  if (k_begin < k_end) load(k_begin);
  for (int k0 = k_begin; k0 < k_end; k0 += kKT) {
#pragma unroll
    for (int r = 0; r < kRB; ++r) {
      s_a[lk][li + 16 * r] = ra[r];
      s_b[lk][li + 16 * r] = rb[r];
    }
    __syncthreads();
    if (k0 + kKT < k_end) load(k0 + kKT);
#if ERPL_SUR_MFMA
    // wave w owns the 64 x 64 quarter (w >> 1, w & 1) of the tile as 4 x 4 blocks of 16 x 16; per 4 members one
    // v_mfma_f64_16x16x4_f64 per block: lane l hands in row (l & 15) of the block at member (l >> 4) on either side
    const int lane = tid & 63, wr = (tid >> 7) * 64, wc = ((tid >> 6) & 1) * 64;
#pragma unroll
    for (int kg = 0; kg < kKT / 4; ++kg) {
      double a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q] = s_a[kg * 4 + (lane >> 4)][wr + q * 16 + (lane & 15)];
        b[q] = s_b[kg * 4 + (lane >> 4)][wc + q * 16 + (lane & 15)];
      }
#pragma unroll
      for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) macc[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], b[bj], macc[bi][bj], 0, 0, 0);
    }
#else
#pragma unroll
    for (int kk = 0; kk < kKT; ++kk) {
      double a[kRB], b[kRB];
#pragma unroll
      for (int i = 0; i < kRB; i += 2) {
        const double2 va = *reinterpret_cast<const double2*>(&s_a[kk][ty * kRB + i]);
        const double2 vb = *reinterpret_cast<const double2*>(&s_b[kk][tx * kRB + i]);
        a[i] = va.x; a[i + 1] = va.y;
        b[i] = vb.x; b[i + 1] = vb.y;
      }
#pragma unroll
      for (int i = 0; i < kRB; ++i)
#pragma unroll
        for (int j = 0; j < kRB; ++j) acc[i][j] = __builtin_fma(a[i], b[j], acc[i][j]);
    }
#endif
    __syncthreads();
  }
  double* __restrict__ out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(kTile * kTile);
#if ERPL_SUR_MFMA
  {   // result r of block (bi, bj) in lane l: row (l >> 4) + 4 r, column l & 15 of the block
    const int lane = tid & 63, wr = (tid >> 7) * 64, wc = ((tid >> 6) & 1) * 64;
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
      for (int bj = 0; bj < 4; ++bj)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(wr + bi * 16 + (lane >> 4) + 4 * r) * kTile + wc + bj * 16 + (lane & 15)] = macc[bi][bj][r];
  }
#else
#pragma unroll
  for (int i = 0; i < kRB; ++i)
#pragma unroll
    for (int j = 0; j < kRB; j += 2)
      *reinterpret_cast<double2*>(&out[(ty * kRB + i) * kTile + tx * kRB + j]) = make_double2(acc[i][j], acc[i][j + 1]);
#endif
}

// ---- fold: workgroup (64 rows of 4 elements of a tile, pair)
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_sur_fold(const double* __restrict__ part, const int slices, const int cols,
                                                                 const int first, double* __restrict__ gram) {
  const int tiles = (cols + kTile - 1) / kTile;
  int ti = 0, left = blockIdx.y;
  while (left >= tiles - ti) { left -= tiles - ti; ++ti; }
  const int tj = ti + left;
  const int el = blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x;   // < kTile kTile
  const int i = el / kTile, j = el - i * kTile, row = ti * kTile + i, col = tj * kTile + j;
  if (row >= cols || col >= cols) return;
  double* __restrict__ g = gram + (size_t)row * cols + col;
  double acc = first ? 0.0 : *g;
  const size_t step = (size_t)gridDim.y * (size_t)(kTile * kTile);
  const double* __restrict__ p = part + (size_t)blockIdx.y * (size_t)(kTile * kTile) + el;
  for (int s = 0; s < slices; ++s) acc += p[(size_t)s * step];
  *g = acc;
}

// ---- predict: columns 0 .. count - 1 of x (through src, if there is one) -> out[n_rows][ld_out]
__global__ void erpl_sur_predict(const ErplSurModel M, const double* __restrict__ x, int64_t ldx, const uint32_t* __restrict__ src,
                                 int64_t count, double* __restrict__ out, int64_t ld_out) {
  extern __shared__ double s_u[];
  const int T = blockDim.x;
  const int64_t c = (int64_t)blockIdx.x * T + threadIdx.x;
  if (c >= count) return;
  const int64_t col = src ? (int64_t)src[c] : c;
  double* u = s_u + threadIdx.x;
  const bool ok = sur_univariate(M, x, ldx, col, u, T);
  for (int j = 0; j < M.n_rows; ++j)
    out[(int64_t)j * ld_out + c] = ok ? erpl_pce_value(M.coef + (size_t)j * M.n_terms, M.terms, M.n_terms, u, M.degree, T) : (double)NAN;
}

// ---- sums over the dense members.  PASS 0: sum y (fitted), sum y (held out).  PASS 1: sum (y - mean)^2 and sum (y - yhat)^2
// of the fitted, then of the held-out members.  Workgroup (block, row j) -> work->part[j][.][block].
struct ErplSurSums {
  const double* y[ERPL_SUR_MAX_ROWS];   // [n]: through src
  const double* yhat;                   // [n_rows][m]
  const uint32_t* src;
  ErplSurWork* work;
  int64_t m, n_fit, n_val;
  int32_t holdout;
};
template <int PASS>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_sur_sums(const ErplSurSums a) {
  const int j = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ y = a.y[j];
  const double* __restrict__ yh = a.yhat + (size_t)j * (size_t)a.m;
  const double mean_fit = PASS ? a.work->mean[j][0] : 0.0, mean_val = PASS ? a.work->mean[j][1] : 0.0;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < a.m; d += stride) {
    const double yd = y[a.src[d]];
    const bool val = sur_held_out(d, a.holdout);
    if (PASS == 0) {
      if (val) v1 += yd; else v0 += yd;
    } else {
      const double dev = yd - (val ? mean_val : mean_fit), res = yd - yh[d];
      if (val) { v2 += dev * dev; v3 += res * res; } else { v0 += dev * dev; v1 += res * res; }
    }
  }
  block_fold<Add, Add, Add, Add>(v0, v1, v2, v3);
  if (threadIdx.x == 0) {
    a.work->part[j][0][blockIdx.x] = v0; a.work->part[j][1][blockIdx.x] = v1;
    a.work->part[j][2][blockIdx.x] = v2; a.work->part[j][3][blockIdx.x] = v3;
  }
}
// one workgroup per row: the partials of nb workgroups in the fixed order
template <int PASS>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_sur_finish(const ErplSurSums a, const int nb) {
  const int j = blockIdx.x;
  double v0 = thread_partials<Add>(a.work->part[j][0], nb), v1 = thread_partials<Add>(a.work->part[j][1], nb);
  double v2 = thread_partials<Add>(a.work->part[j][2], nb), v3 = thread_partials<Add>(a.work->part[j][3], nb);
  block_fold<Add, Add, Add, Add>(v0, v1, v2, v3);
  if (threadIdx.x != 0) return;
  if (PASS == 0) {
    a.work->mean[j][0] = v0 / (double)a.n_fit;
    a.work->mean[j][1] = v1 / (double)a.n_val;
  } else {
    a.work->out[j][0] = v0; a.work->out[j][1] = v1; a.work->out[j][2] = v2; a.work->out[j][3] = v3;
  }
}

// ---- host
int sur_check_int(int v, const char* name, int lo, int hi) {
  if (v >= lo && v <= hi) return ERPL_OK;
  return erpl_fail(ERPL_ERR_INVALID, "spec->%s = %d outside %d..%d", name, v, lo, hi);
}
int sur_check_n(int64_t n) {
  if (n <= 0) return erpl_fail(ERPL_ERR_INVALID, "n = %lld: need at least one sample", (long long)n);
  if (n >= ((int64_t)1 << 31)) return erpl_fail(ERPL_ERR_INVALID, "n = %lld: sample indices are carried in 31 bits", (long long)n);
  return ERPL_OK;
}
// n_vars, n_rows, degree, order of a spec, in this order
int sur_check_shape(const erpl_sur_spec* s) {
  ERPL_TRY(sur_check_int(s->n_vars, "n_vars", 1, ERPL_SUR_MAX_VARS));
  ERPL_TRY(sur_check_int(s->n_rows, "n_rows", 1, ERPL_SUR_MAX_ROWS));
  ERPL_TRY(sur_check_int(s->degree, "degree", 1, ERPL_SUR_MAX_DEGREE));
  return sur_check_int(s->order, "order", 1, ERPL_SUR_MAX_ORDER);
}
int sur_check_kinds(const uint8_t* kinds, int n_vars) {
  for (int v = 0; v < n_vars; ++v)
    if (kinds[v] != ERPL_DESIGN_UNIFORM && kinds[v] != ERPL_DESIGN_NORMAL)
      return erpl_fail(ERPL_ERR_INVALID, "kinds[%d] = %d is neither ERPL_DESIGN_UNIFORM nor ERPL_DESIGN_NORMAL", v, (int)kinds[v]);
  return ERPL_OK;
}
int sur_check_terms(int n_vars, int degree, int order, int* P) {
  const int64_t p = erpl_pce_count(n_vars, degree, order);
  if (p > ERPL_SUR_MAX_TERMS)
    return erpl_fail(ERPL_ERR_INVALID, "n_vars = %d, degree = %d, order = %d give %lld terms, above ERPL_SUR_MAX_TERMS = %d", n_vars,
                     degree, order, (long long)p, ERPL_SUR_MAX_TERMS);
  *P = (int)p;
  return ERPL_OK;
}
// the refusals erpl_mc_surrogate_predict and _predict_host share, in the order of the header
int sur_check_predict(const erpl_sur_spec* s, const uint8_t* kinds, const double* coef, const double* X, int64_t ld, int64_t n,
                      const double* out, int* P) {
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (!kinds) return erpl_fail(ERPL_ERR_INVALID, "kinds is NULL");
  if (!coef) return erpl_fail(ERPL_ERR_INVALID, "coefficients is NULL");
  if (!X) return erpl_fail(ERPL_ERR_INVALID, "X is NULL");
  if (!out) return erpl_fail(ERPL_ERR_INVALID, "out is NULL");
  ERPL_TRY(sur_check_n(n));
  ERPL_TRY(sur_check_shape(s));
  ERPL_TRY(sur_check_kinds(kinds, s->n_vars));
  ERPL_TRY(sur_check_terms(s->n_vars, s->degree, s->order, P));
  if (ld < n) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below n = %lld", (long long)ld, (long long)n);
  return ERPL_OK;
}

// tables, kinds, terms (and, if there are any, coefficients) as the model piece of a device buffer holds them
void sur_pack_model(const ErplSurLayout& at, const uint8_t* kinds, int V, int R, int P, const int8_t* terms, const double* coef,
                    std::vector<char>& blob) {
  blob.assign(at.model_bytes, 0);
  ErplPceTables tab;
  erpl_pce_make_tables(&tab);
  memcpy(blob.data(), &tab, sizeof(tab));
  memcpy(blob.data() + at.m_kinds, kinds, (size_t)V);
  memcpy(blob.data() + at.m_terms, terms, (size_t)P * kTermBytes);
  if (coef) memcpy(blob.data() + at.m_coef, coef, (size_t)R * P * sizeof(double));
}
ErplSurModel sur_model_at(const char* base, const ErplSurLayout& at, int V, int R, int degree, int P) {
  ErplSurModel M;
  M.tab = (const ErplPceTables*)base;
  M.kinds = (const uint8_t*)(base + at.m_kinds);
  M.terms = (const int8_t*)(base + at.m_terms);
  M.coef = (const double*)(base + at.m_coef);
  M.n_vars = V; M.n_rows = R; M.degree = degree; M.n_terms = P;
  return M;
}

// Cholesky of the symmetric G (P x P, row-major, read in its lower triangle) into L (lower, row-major).  Returns false at
// the first pivot that is not finite and > 0; *lo / *hi: the smallest and largest pivot met.
bool sur_cholesky(const std::vector<double>& G, int P, std::vector<double>& L, double* lo, double* hi) {
  L.assign((size_t)P * P, 0.0);
  *lo = INFINITY; *hi = -INFINITY;
  for (int j = 0; j < P; ++j) {
    const double* lj = &L[(size_t)j * P];
    double d = G[(size_t)j * P + j];
    for (int k = 0; k < j; ++k) d -= lj[k] * lj[k];
    if (d != d) { *lo = *hi = d; return false; }
    if (d < *lo) *lo = d;
    if (d > *hi) *hi = d;
    if (!(std::isfinite(d) && d > 0.0)) return false;
    const double root = sqrt(d);
    L[(size_t)j * P + j] = root;
    for (int i = j + 1; i < P; ++i) {
      double* li = &L[(size_t)i * P];
      double s = G[(size_t)i * P + j];
      for (int k = 0; k < j; ++k) s -= li[k] * lj[k];
      li[j] = s / root;
    }
  }
  return true;
}
// L L^T c = b
void sur_solve(const std::vector<double>& L, int P, const double* b, double* c) {
  for (int i = 0; i < P; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[(size_t)i * P + k] * c[k];
    c[i] = s / L[(size_t)i * P + i];
  }
  for (int i = P - 1; i >= 0; --i) {
    double s = c[i];
    for (int k = i + 1; k < P; ++k) s -= L[(size_t)k * P + i] * c[k];
    c[i] = s / L[(size_t)i * P + i];
  }
}

// mean, variance_pce, first, total and the pair indices of one row from its coefficients, in ascending term index
void sur_indices(const double* c, const int8_t* terms, int P, int V, erpl_sur_row* o, double* pair) {
  double var = 0.0, first[ERPL_SUR_MAX_VARS] = {}, total[ERPL_SUR_MAX_VARS] = {};
  if (pair) std::fill(pair, pair + (size_t)V * V, 0.0);
  for (int t = 1; t < P; ++t) {
    const int8_t* tm = terms + (size_t)t * kTermBytes;
    const double sq = c[t] * c[t];
    var += sq;
    int used = 0;
    for (int s = 0; s < ERPL_PCE_SLOTS && tm[2 * s] >= 0; ++s) { total[tm[2 * s]] += sq; ++used; }
    if (used == 1) first[tm[0]] += sq;
    if (used == 2 && pair) pair[(size_t)tm[0] * V + tm[2]] += sq;
  }
  o->mean = c[0];
  o->variance_pce = var;
  const bool any = var != 0.0;   // a NaN variance divides into NaN by itself
  for (int v = 0; v < V; ++v) {
    o->first[v] = any ? first[v] / var : (double)NAN;
    o->total[v] = any ? total[v] / var : (double)NAN;
  }
  if (pair && !any) std::fill(pair, pair + (size_t)V * V, (double)NAN);   // the diagonal too, as after a fit that failed
  if (pair && any)
    for (int i = 0; i < V; ++i)
      for (int k = i + 1; k < V; ++k) {
        const double share = any ? pair[(size_t)i * V + k] / var : (double)NAN;
        pair[(size_t)i * V + k] = pair[(size_t)k * V + i] = share;
      }
}

}  // namespace

extern "C" {

int erpl_mc_surrogate_defaults(erpl_sur_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  memset(spec, 0, sizeof(*spec));
  spec->n_rows = 3;
  spec->rows[0] = ERPL_SUM_APOGEE_ALT; spec->rows[1] = ERPL_SUM_RANGE; spec->rows[2] = ERPL_SUM_FLIGHT_TIME;
  spec->degree = 2;
  spec->order = 2;
  return ERPL_OK;
}

int erpl_mc_surrogate_terms(int32_t n_vars, int32_t degree, int32_t order, int32_t* n_terms, int8_t* terms) {
  if (!n_terms) return erpl_fail(ERPL_ERR_INVALID, "n_terms is NULL");
  erpl_sur_spec s = {};
  s.n_vars = n_vars; s.n_rows = 1; s.degree = degree; s.order = order;
  ERPL_TRY(sur_check_shape(&s));
  int P = 0;
  ERPL_TRY(sur_check_terms(n_vars, degree, order, &P));
  *n_terms = P;
  if (terms && erpl_pce_enumerate(n_vars, degree, order, terms, P) != P)
    return erpl_fail(ERPL_ERR_INTERNAL, "erpl_mc_surrogate_terms: the enumeration and the closed form disagree");
  return ERPL_OK;
}

int erpl_mc_surrogate_predict_host(const erpl_sur_spec* spec, const uint8_t* kinds, const double* coefficients, const double* X,
                                   int64_t ld, int64_t n, double* out) {
  int P = 0;
  ERPL_TRY(sur_check_predict(spec, kinds, coefficients, X, ld, n, out, &P));
  const int V = spec->n_vars, R = spec->n_rows, degree = spec->degree;
  std::vector<int8_t> terms((size_t)P * kTermBytes);
  erpl_pce_enumerate(V, degree, spec->order, terms.data(), P);
  ErplPceTables tab;
  erpl_pce_make_tables(&tab);
  const int nthr = host_threads(0, n);
  run_threads(nthr, [&](int w) {
    std::vector<double> u((size_t)V * degree);
    for (int64_t c = n * w / nthr; c < n * (w + 1) / nthr; ++c) {
      bool ok = true;
      for (int v = 0; v < V; ++v) {
        const double xv = X[(int64_t)v * ld + c];
        ok = ok && erpl_pce_finite(xv);
        erpl_pce_univariate(tab, kinds[v], xv, degree, u.data() + (size_t)v * degree, 1);
      }
      for (int j = 0; j < R; ++j)
        out[(int64_t)j * ld + c] = ok ? erpl_pce_value(coefficients + (size_t)j * P, terms.data(), P, u.data(), degree, 1) : (double)NAN;
    }
  });
  return ERPL_OK;
}

int erpl_mc_surrogate_predict(erpl_ctx* c, const erpl_sur_spec* spec, const uint8_t* kinds, const double* coefficients, const double* X,
                              int64_t ld, int64_t n, double* out, void* stream) {
  int P = 0;
  ERPL_TRY(sur_check_predict(spec, kinds, coefficients, X, ld, n, out, &P));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int V = spec->n_vars, R = spec->n_rows, degree = spec->degree;
  std::vector<int8_t> terms((size_t)P * kTermBytes);
  erpl_pce_enumerate(V, degree, spec->order, terms.data(), P);
  ErplSurLayout at = {};
  erpl_sur_model_pieces(R, P, &at);
  std::vector<char> blob;
  sur_pack_model(at, kinds, V, R, P, terms.data(), coefficients, blob);
  ERPL_TRY(c->sur_model.grow(at.model_bytes));
  // through pinned staging, so that the copy does not wait for the stream: the staging is free once the copy before has run
  if (!c->sur_ev) HIP_TRY(hipEventCreateWithFlags(&c->sur_ev, hipEventDisableTiming));
  else HIP_TRY(hipEventSynchronize(c->sur_ev));
  if (at.model_bytes > c->sur_pin_cap) {
    if (c->sur_pin) (void)hipHostFree(c->sur_pin);
    c->sur_pin = nullptr; c->sur_pin_cap = 0;
    HIP_TRY(hipHostMalloc((void**)&c->sur_pin, at.model_bytes, hipHostMallocDefault));
    c->sur_pin_cap = at.model_bytes;
  }
  memcpy(c->sur_pin, blob.data(), at.model_bytes);
  HIP_TRY(hipMemcpyAsync(c->sur_model.buf, c->sur_pin, at.model_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(c->sur_ev, st));
  const ErplSurModel M = sur_model_at(c->sur_model.buf, at, V, R, degree, P);
  const int T = erpl_sur_group(V, degree);
  hipLaunchKernelGGL(erpl_sur_predict, dim3((unsigned)((n + T - 1) / T)), dim3(T), (size_t)T * V * degree * sizeof(double), st, M, X, ld,
                     (const uint32_t*)nullptr, n, out, ld);
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

int erpl_mc_surrogate(erpl_ctx* c, const double* factors, const uint8_t* kinds, const double* summary, const double* extra,
                      const uint8_t* mask, int64_t n, const erpl_sur_spec* spec, erpl_surrogate* result, double* coefficients,
                      int8_t* terms_out, double* gram_out, double* rhs_out, double* pair_out, void* stream) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (!factors) return erpl_fail(ERPL_ERR_INVALID, "factors is NULL");
  if (!kinds) return erpl_fail(ERPL_ERR_INVALID, "kinds is NULL");
  if (!summary) return erpl_fail(ERPL_ERR_INVALID, "summary is NULL");
  if (!result) return erpl_fail(ERPL_ERR_INVALID, "result is NULL");
  if (!coefficients) return erpl_fail(ERPL_ERR_INVALID, "coefficients is NULL");
  ERPL_TRY(sur_check_n(n));
  ERPL_TRY(sur_check_shape(spec));
  if (spec->holdout != 0 && !(spec->holdout >= 2 && spec->holdout <= ERPL_SUR_MAX_HOLDOUT))
    return erpl_fail(ERPL_ERR_INVALID, "spec->holdout = %d is neither 0 nor in 2..%d", spec->holdout, ERPL_SUR_MAX_HOLDOUT);
  ERPL_TRY(sur_check_kinds(kinds, spec->n_vars));
  const int V = spec->n_vars, R = spec->n_rows, degree = spec->degree, holdout = spec->holdout;
  for (int j = 0; j < R; ++j) {
    if (spec->rows[j] < 0 || spec->rows[j] > ERPL_SUR_ROW_EXTRA)
      return erpl_fail(ERPL_ERR_INVALID, "spec->rows[%d] = %d outside 0..%d", j, spec->rows[j], ERPL_SUR_ROW_EXTRA);
    for (int k = 0; k < j; ++k)
      if (spec->rows[k] == spec->rows[j]) return erpl_fail(ERPL_ERR_INVALID, "spec->rows[%d] = %d is listed twice", j, spec->rows[j]);
  }
  for (int j = 0; j < R; ++j)
    if (spec->rows[j] == ERPL_SUR_ROW_EXTRA && !extra)
      return erpl_fail(ERPL_ERR_INVALID, "extra is NULL but spec->rows[%d] = %d (ERPL_SUR_ROW_EXTRA)", j, spec->rows[j]);
  int P = 0;
  ERPL_TRY(sur_check_terms(V, degree, spec->order, &P));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int cols = P + R;
  const size_t un = (size_t)n, uP = (size_t)P;

  std::vector<int8_t> terms(uP * kTermBytes);
  erpl_pce_enumerate(V, degree, spec->order, terms.data(), P);
  if (terms_out) memcpy(terms_out, terms.data(), terms.size());

  size_t temp_bytes = 0;
  LAUNCH_TRY(erpl_boot_select_bytes(n, &temp_bytes), "select sizing failed");
  const ErplSurLayout at = erpl_sur_layout(n, R, P, temp_bytes);
  ERPL_TRY(c->corr.first_use());   // the population pass and its counters
  ERPL_TRY(c->sur.first_use());
  ERPL_TRY(c->sur.grow(at.need));
  char* buf = c->sur.buf;
  SurHost& h = *c->sur.host;

  ErplSurRows rows = {};
  const double** yrow = rows.y;
  ErplCorrArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.mask = mask; pa.n = n; pa.n_vars = V + R; pa.work = c->corr.work; pa.pop = (uint8_t*)(buf + at.pop);
  for (int v = 0; v < V; ++v) pa.var[v] = factors + (size_t)v * un;
  for (int j = 0; j < R; ++j) {
    yrow[j] = spec->rows[j] == ERPL_SUR_ROW_EXTRA ? extra : summary + (size_t)spec->rows[j] * un;
    pa.var[V + j] = yrow[j];
  }
  KERNEL_TRY(erpl_launch_corr_population(pa, stream));
  HIP_TRY(hipMemcpyAsync(h.counter, &c->corr.work->out.counter[0], sizeof(h.counter), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t m = (int64_t)h.counter[0];
  const int64_t n_val = holdout ? m / holdout : 0, n_fit = m - n_val;

  const double nan = NAN;
  memset(result, 0, sizeof(*result));
  result->n = n; result->count = m; result->n_masked = (int64_t)h.counter[1]; result->n_non_finite = (int64_t)h.counter[2];
  result->n_fit = n_fit; result->n_val = n_val;
  result->n_vars = V; result->n_rows = R; result->degree = degree; result->order = spec->order; result->holdout = holdout;
  result->n_terms = P;
  result->pivot_min = result->pivot_max = nan;
  for (int j = 0; j < ERPL_SUR_MAX_ROWS; ++j) {
    erpl_sur_row& o = result->row[j];
    o.mean = o.variance_pce = o.tss_fit = o.rss_fit = o.r2 = o.tss_val = o.rss_val = o.q2 = nan;
    for (int v = 0; v < ERPL_SUR_MAX_VARS; ++v) o.first[v] = o.total[v] = nan;
  }
  std::fill(coefficients, coefficients + (size_t)R * uP, nan);
  if (pair_out) std::fill(pair_out, pair_out + (size_t)R * V * V, nan);

  // the model without coefficients (`blob` outlives the copy: every path with members synchronises the stream below)
  std::vector<char> blob;
  const ErplSurModel M = sur_model_at(buf + at.model, at, V, R, degree, P);
  uint32_t* src = (uint32_t*)(buf + at.src);
  if (m > 0) {
    sur_pack_model(at, kinds, V, R, P, terms.data(), nullptr, blob);
    HIP_TRY(hipMemcpyAsync(buf + at.model, blob.data(), at.model_bytes, hipMemcpyHostToDevice, st));
    ErplBootPrep p;
    memset(&p, 0, sizeof(p));
    p.pop = pa.pop; p.src = src; p.count = (unsigned long long*)(buf + at.count);
    p.temp = buf + at.temp; p.temp_bytes = at.temp_bytes; p.n = n;
    LAUNCH_TRY(erpl_launch_boot_compact(p, stream), "select failed");
  }

  // G and b: chunk after chunk
  double* A = (double*)(buf + at.psi);
  double* part = (double*)(buf + at.part);
  double* gram = (double*)(buf + at.gram);
  const int T = erpl_sur_group(V, degree), pairs = erpl_sur_pairs(cols);
  const size_t u_bytes = (size_t)T * V * degree * sizeof(double);
  std::vector<double> aug((size_t)cols * cols, 0.0);   // A A^T: G, b and the squares of the rows
  for (int64_t e0 = 0; e0 < n_fit; e0 += ERPL_SUR_CHUNK) {
    const int len = (int)std::min<int64_t>(ERPL_SUR_CHUNK, n_fit - e0);   // <= at.ld: n_fit <= n
    int slice_len = 0;
    const int slices = erpl_sur_slices(len, P, &slice_len);
    if (slices > at.slices)   // cannot be: at.slices = erpl_sur_max_slices(at.ld, P) bounds every chunk of at most at.ld members
      return erpl_fail(ERPL_ERR_INTERNAL, "erpl_mc_surrogate: %d slices of a chunk of %d members, room for %d", slices, len, at.slices);
    hipLaunchKernelGGL(erpl_sur_basis, dim3((unsigned)((len + T - 1) / T)), dim3(T), u_bytes, st, M, factors, rows, n, src, holdout, e0,
                       len, A, at.ld);
    hipLaunchKernelGGL(erpl_sur_gram, dim3(pairs, slices), dim3(256), 0, st, A, at.ld, cols, len, slice_len, part);
    hipLaunchKernelGGL(erpl_sur_fold, dim3(kTile * kTile / ERPL_ANA_BLOCK, pairs), dim3(ERPL_ANA_BLOCK), 0, st, part, slices, cols,
                       e0 == 0 ? 1 : 0, gram);
    HIP_TRY(hipGetLastError());
  }
  if (n_fit > 0) {
    HIP_TRY(hipMemcpyAsync(aug.data(), gram, aug.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  std::vector<double> G(uP * uP), rhs((size_t)R * uP);
  for (int i = 0; i < P; ++i)
    for (int k = i; k < P; ++k) G[(size_t)i * P + k] = G[(size_t)k * P + i] = aug[(size_t)i * cols + k];
  for (int j = 0; j < R; ++j)
    for (int i = 0; i < P; ++i) rhs[(size_t)j * P + i] = aug[(size_t)i * cols + P + j];
  if (gram_out) memcpy(gram_out, G.data(), G.size() * sizeof(double));
  if (rhs_out) memcpy(rhs_out, rhs.data(), rhs.size() * sizeof(double));

  // the solve
  bool fit_ok = false;
  if (n_fit > 0) {
    std::vector<double> L;
    const bool factored = sur_cholesky(G, P, L, &result->pivot_min, &result->pivot_max);
    fit_ok = factored && n_fit >= P;
    if (fit_ok)
      for (int j = 0; j < R; ++j) sur_solve(L, P, rhs.data() + (size_t)j * P, coefficients + (size_t)j * P);
  }
  for (int j = 0; j < R; ++j) result->row[j].fit_ok = fit_ok ? 1 : 0;
  if (m == 0) return ERPL_OK;

  // the residuals
  HIP_TRY(hipMemcpyAsync(buf + at.model + at.m_coef, coefficients, (size_t)R * uP * sizeof(double), hipMemcpyHostToDevice, st));
  double* yhat = (double*)(buf + at.yhat);
  hipLaunchKernelGGL(erpl_sur_predict, dim3((unsigned)((m + T - 1) / T)), dim3(T), u_bytes, st, M, factors, n, (const uint32_t*)src, m, yhat,
                     m);
  ErplSurSums sa;
  memset(&sa, 0, sizeof(sa));
  for (int j = 0; j < R; ++j) sa.y[j] = yrow[j];
  sa.yhat = yhat; sa.src = src; sa.work = c->sur.work; sa.m = m; sa.n_fit = n_fit; sa.n_val = n_val; sa.holdout = holdout;
  const int nb = grid_of(m);
  hipLaunchKernelGGL(erpl_sur_sums<0>, dim3(nb, R), dim3(ERPL_ANA_BLOCK), 0, st, sa);
  hipLaunchKernelGGL(erpl_sur_finish<0>, dim3(R), dim3(ERPL_ANA_BLOCK), 0, st, sa, nb);
  hipLaunchKernelGGL(erpl_sur_sums<1>, dim3(nb, R), dim3(ERPL_ANA_BLOCK), 0, st, sa);
  hipLaunchKernelGGL(erpl_sur_finish<1>, dim3(R), dim3(ERPL_ANA_BLOCK), 0, st, sa, nb);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h.out, c->sur.work->out, sizeof(h.out), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  for (int j = 0; j < R; ++j) {
    erpl_sur_row& o = result->row[j];
    o.tss_fit = n_fit > 0 ? h.out[j][0] : nan; o.rss_fit = n_fit > 0 ? h.out[j][1] : nan;
    o.r2 = o.tss_fit == 0.0 ? nan : 1.0 - o.rss_fit / o.tss_fit;
    if (n_val > 0) {
      o.tss_val = h.out[j][2]; o.rss_val = h.out[j][3];
      o.q2 = o.tss_val == 0.0 ? nan : 1.0 - o.rss_val / o.tss_val;
    }
    if (fit_ok) sur_indices(coefficients + (size_t)j * P, terms.data(), P, V, &o, pair_out ? pair_out + (size_t)j * V * V : nullptr);
  }
  return ERPL_OK;
}

}  // extern "C"
