// erpl_distributions.hip — the device passes of erpl_mc_histogram, erpl_mc_histogram_xy and erpl_mc_dispersion: what
// MonteCarloAnalyzer.plot_results of the reference draws from Python lists (monte_carlo.py:562-633) and the landing
// dispersion, as reductions over the [16][n] summary next to erpl_mc_analyze.
//
// Every pass streams its rows once, coalesced, on the grid of the analysis passes (a function of n alone):
//   range      masked min / max of the rows whose range comes from the data; partials per workgroup, no atomics
//   hist       one row per grid.y: the row's edges (written by the host, np.linspace's arithmetic) and a 32-bit count per
//              bin in LDS; every lane corrects NumPy's guessed bin against the edges; flushed with 64-bit integer atomics
//   hist2d     the same per axis; an LDS tile for grids of up to ERPL_DIST_TILE_CELLS cells, global integer atomics above
//   dispersion two moment passes over two rows (mean, then the sums about it), then one pass that counts the content of
//              every confidence ellipse with ballots and writes the miss distance the selection of erpl_analysis.hip reads
// Sums are accumulated per thread in index order and reduced in the fixed order of erpl_stat_device.h; integer adds commute:
// the same bits in every call.  No floating-point atomics.  Compiled with -ffp-contract=off: the guess, (x - mean)^2 and
// dx*dx + dy*dy are rounded as NumPy rounds them.
#include "erpl_stat_device.h"
#include "erpl_tally.h"

namespace {

// the bin of x among the edge values e[0..bins]: np.histogram's rule, defined once for these kernels and the tally (erpl_tally.h)
__device__ __forceinline__ int bin_of(double x, double lo, double hi, int bins, const double* e) {
  return erpl_bin_of(x, lo, hi, bins, e);
}

// ---- range: min / max of row rows[blockIdx.y] over the samples that count
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dist_range(const ErplDistArgs a) {
  const int j = blockIdx.y;
  if (!a.automatic[j]) return;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.rows[j] * n;
  const double* __restrict__ y = a.partner[j] >= 0 ? a.summary + (int64_t)a.partner[j] * n : nullptr;
  const uint8_t* __restrict__ mask = a.mask;
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < n; i += stride) {
    const double v = x[i];
    bool use = finite_bits(v) && (!mask || mask[i] == 0);
    if (y) use = use && finite_bits(y[i]);
    if (use) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
  }
  block_fold<Min, Max>(mn, mx);
  if (threadIdx.x == 0) {
    a.work->pmin[j][blockIdx.x] = mn;
    a.work->pmax[j][blockIdx.x] = mx;
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dist_finish_range(const ErplDistArgs a, const int nb) {
  const int j = blockIdx.x;
  if (!a.automatic[j]) return;
  double mn = thread_partials<Min>(a.work->pmin[j], nb), mx = thread_partials<Max>(a.work->pmax[j], nb);
  block_fold<Min, Max>(mn, mx);
  if (threadIdx.x == 0) {
    a.work->range.lo[j] = mn;   // +inf / -inf: nothing counted
    a.work->range.hi[j] = mx;
  }
}

// ---- hist: row rows[blockIdx.y] into its bins
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dist_hist(const ErplDistArgs a) {
  __shared__ double s_edge[ERPL_HIST_MAX_BINS + 1];
  __shared__ unsigned int s_cnt[ERPL_HIST_MAX_BINS];
  const int j = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bins = a.bins[j];
  const double lo = a.lo[j], hi = a.hi[j];
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.rows[j] * n;
  const uint8_t* __restrict__ mask = a.mask;
  for (int k = threadIdx.x; k <= bins; k += ERPL_ANA_BLOCK) s_edge[k] = a.work->edges[j][k];
  for (int k = threadIdx.x; k < bins; k += ERPL_ANA_BLOCK) s_cnt[k] = 0u;
  __syncthreads();
  u64 tot[3] = {0ull, 0ull, 0ull};   // counted, below, above: uniform over the wave
  for (int64_t base = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    bool use = false;
    double v = 0.0;
    if (i < n) {
      v = x[i];
      use = finite_bits(v) && (!mask || mask[i] == 0);
    }
    const bool lt = use && v < lo, gt = use && v > hi, hit = use && !lt && !gt;
    tot[0] += __popcll(__ballot(use));
    tot[1] += __popcll(__ballot(lt));
    tot[2] += __popcll(__ballot(gt));
    const u64 m = __ballot(hit);
    if (m == 0ull) continue;
    const int k = hit ? bin_of(v, lo, hi, bins, s_edge) : 0;
    // a constant row or heavily tied data puts a whole wave into one bin: one add of the lane count
    const int lead = __ffsll((long long)m) - 1;
    const int k0 = __shfl(k, lead);
    if (__ballot(hit && k != k0) == 0ull) {
      if (lane == lead) atomicAdd(&s_cnt[k0], (unsigned int)__popcll(m));
    } else if (hit) {
      atomicAdd(&s_cnt[k], 1u);
    }
  }
  const u64 s = counters_fold(tot);   // behind its barrier s_cnt is complete
  ErplDistHist& h = a.work->hist;
  for (int k = threadIdx.x; k < bins; k += ERPL_ANA_BLOCK) {
    const unsigned int c = s_cnt[k];
    if (c) atomicAdd(&h.bins[j][k], (u64)c);
  }
  if (threadIdx.x < 3) {
    u64* dst = threadIdx.x == 0 ? &h.counted[j] : (threadIdx.x == 1 ? &h.below[j] : &h.above[j]);
    if (s) atomicAdd(dst, s);
  }
}

// ---- hist2d: rows[0] x rows[1] into bins[0] x bins[1] cells, x-major.  TILE: the cells of this workgroup in LDS.
template <bool TILE>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dist_hist2d(const ErplDistArgs a) {
  __shared__ double s_ex[ERPL_HIST2D_MAX_BINS + 1], s_ey[ERPL_HIST2D_MAX_BINS + 1];
  __shared__ unsigned int s_cnt[TILE ? ERPL_DIST_TILE_CELLS : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bx = a.bins[0], by = a.bins[1], cells = bx * by;
  const double lox = a.lo[0], hix = a.hi[0], loy = a.lo[1], hiy = a.hi[1];
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.rows[0] * n;
  const double* __restrict__ y = a.summary + (int64_t)a.rows[1] * n;
  const uint8_t* __restrict__ mask = a.mask;
  for (int k = threadIdx.x; k <= bx; k += ERPL_ANA_BLOCK) s_ex[k] = a.work->edges[0][k];
  for (int k = threadIdx.x; k <= by; k += ERPL_ANA_BLOCK) s_ey[k] = a.work->edges[1][k];
  if (TILE) for (int k = threadIdx.x; k < cells; k += ERPL_ANA_BLOCK) s_cnt[k] = 0u;
  __syncthreads();
  u64 tot[2] = {0ull, 0ull};   // counted, outside: uniform over the wave
  for (int64_t base = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    bool use = false;
    double vx = 0.0, vy = 0.0;
    if (i < n) {
      vx = x[i]; vy = y[i];
      use = finite_bits(vx) && finite_bits(vy) && (!mask || mask[i] == 0);
    }
    const bool hit = use && vx >= lox && vx <= hix && vy >= loy && vy <= hiy;
    tot[0] += __popcll(__ballot(use));
    tot[1] += __popcll(__ballot(use && !hit));
    const u64 m = __ballot(hit);
    if (m == 0ull) continue;
    const int c = hit ? bin_of(vx, lox, hix, bx, s_ex) * by + bin_of(vy, loy, hiy, by, s_ey) : 0;
    const int lead = __ffsll((long long)m) - 1;
    const int c0 = __shfl(c, lead);
    if (__ballot(hit && c != c0) == 0ull) {
      if (lane == lead) {
        if (TILE) atomicAdd(&s_cnt[c0], (unsigned int)__popcll(m));
        else atomicAdd(&a.work->cells[c0], (u64)__popcll(m));
      }
    } else if (hit) {
      if (TILE) atomicAdd(&s_cnt[c], 1u);
      else atomicAdd(&a.work->cells[c], 1ull);
    }
  }
  const u64 s = counters_fold(tot);   // behind its barrier s_cnt is complete
  if (TILE)
    for (int k = threadIdx.x; k < cells; k += ERPL_ANA_BLOCK) {
      const unsigned int c = s_cnt[k];
      if (c) atomicAdd(&a.work->cells[k], (u64)c);
    }
  if (threadIdx.x < 2 && s) atomicAdd(threadIdx.x == 0 ? &a.work->counted2 : &a.work->outside2, s);
}

// ---- dispersion moments.  SECOND = false: sums of x and y and the count over the samples that count; SECOND = true:
// sums of dx dx, dx dy, dy dy about the mean of the first pass.
template <bool SECOND>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_disp_moments(const ErplDispArgs a) {
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.row_x * n;
  const double* __restrict__ y = a.summary + (int64_t)a.row_y * n;
  const uint8_t* __restrict__ mask = a.mask;
  const double mx = SECOND ? a.work->mom.mean_x : 0.0, my = SECOND ? a.work->mom.mean_y : 0.0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  u64 cnt = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < n; i += stride) {
    const double vx = x[i], vy = y[i];
    if (finite_bits(vx) && finite_bits(vy) && (!mask || mask[i] == 0)) {
      if (SECOND) {
        const double dx = vx - mx, dy = vy - my;
        s0 += dx * dx; s1 += dx * dy; s2 += dy * dy;
      } else {
        s0 += vx; s1 += vy; ++cnt;
      }
    }
  }
  if (SECOND) block_fold<Add, Add, Add>(s0, s1, s2);
  else block_fold<Add, Add, Add>(s0, s1, cnt);
  if (threadIdx.x == 0) {
    a.work->dsum[0][blockIdx.x] = s0;
    a.work->dsum[1][blockIdx.x] = s1;
    if (SECOND) a.work->dsum[2][blockIdx.x] = s2;
    else a.work->dcnt[blockIdx.x] = cnt;
  }
}

template <bool SECOND>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_disp_finish(const ErplDispArgs a, const int nb) {
  ErplDistWork* w = a.work;
  double s0 = thread_partials<Add>(w->dsum[0], nb), s1 = thread_partials<Add>(w->dsum[1], nb);
  double s2 = SECOND ? thread_partials<Add>(w->dsum[2], nb) : 0.0;
  u64 cnt = SECOND ? 0ull : thread_partials<Add>(w->dcnt, nb);
  if (SECOND) block_fold<Add, Add, Add>(s0, s1, s2);
  else block_fold<Add, Add, Add>(s0, s1, cnt);
  if (threadIdx.x != 0) return;
  ErplDistMoments& m = w->mom;
  if (!SECOND) {
    m.count = cnt;
    m.mean_x = s0 / (double)cnt;   // NaN for an empty cloud; the host reports every double of it as NaN
    m.mean_y = s1 / (double)cnt;
  } else {
    const double c = (double)m.count;
    m.sxx = s0; m.sxy = s1; m.syy = s2;
    m.cov_xx = s0 / c; m.cov_xy = s1 / c; m.cov_yy = s2 / c;
    m.det = m.cov_xx * m.cov_yy - m.cov_xy * m.cov_xy;
    m.centre_x = a.centre == ERPL_CENTRE_POINT ? a.cx : m.mean_x;
    m.centre_y = a.centre == ERPL_CENTRE_POINT ? a.cy : m.mean_y;
  }
}

// ---- the content of every confidence ellipse (ballots: the counts of a wave are uniform; the workgroup's go to its own
// slot of work->ipart) and the miss distance of every sample
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_disp_inside(const ErplDispArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.row_x * n;
  const double* __restrict__ y = a.summary + (int64_t)a.row_y * n;
  const uint8_t* __restrict__ mask = a.mask;
  const ErplDistMoments& m = a.work->mom;
  const double mx = m.mean_x, my = m.mean_y, cxx = m.cov_xx, cxy = m.cov_xy, cyy = m.cov_yy, det = m.det;
  const double ox = m.centre_x, oy = m.centre_y;
  const bool solid = det > 0.0 && finite_bits(det);
  u64 in[ERPL_DISP_MAX_LEVELS];
#pragma unroll
  for (int k = 0; k < ERPL_DISP_MAX_LEVELS; ++k) in[k] = 0ull;
  for (int64_t base = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    bool use = false;
    double d2 = 0.0;
    if (i < n) {
      const double vx = x[i], vy = y[i];
      use = finite_bits(vx) && finite_bits(vy) && (!mask || mask[i] == 0);
      double r = NAN;
      if (use) {
        const double dx = vx - mx, dy = vy - my;
        d2 = (cyy * dx * dx - 2.0 * cxy * dx * dy + cxx * dy * dy) / det;
        const double ex = vx - ox, ey = vy - oy;
        r = sqrt(ex * ex + ey * ey);
      }
      a.miss[i] = r;
    }
    if (solid) {
#pragma unroll
      for (int k = 0; k < ERPL_DISP_MAX_LEVELS; ++k)
        if (k < a.n_levels) in[k] += __popcll(__ballot(use && d2 <= a.k2[k]));
    }
  }
  const u64 s = counters_fold(in);
  if (threadIdx.x < ERPL_DISP_MAX_LEVELS) a.work->ipart[blockIdx.x][threadIdx.x] = s;
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_disp_finish_inside(const ErplDispArgs a, const int nb) {
  for (int k = 0; k < ERPL_DISP_MAX_LEVELS; ++k) {
    u64 s = thread_partials<Add>(&a.work->ipart[0][k], nb, ERPL_DISP_MAX_LEVELS);
    block_fold_again<Add>(s);   // the same scratch in every round
    if (threadIdx.x == 0) a.work->mom.inside[k] = s;
  }
}

}  // namespace

int erpl_launch_dist_range(const ErplDistArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);
  hipLaunchKernelGGL(erpl_dist_range, dim3(nb, a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(erpl_dist_finish_range, dim3(a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a, nb);
  return (int)hipGetLastError();
}

int erpl_launch_dist_hist(const ErplDistArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(&a.work->hist, 0, sizeof(a.work->hist), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(erpl_dist_hist, dim3(grid_of(a.n), a.n_rows), dim3(ERPL_ANA_BLOCK), 0, st, a);
  return (int)hipGetLastError();
}

int erpl_launch_dist_hist2d(const ErplDistArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t cells = (size_t)a.bins[0] * (size_t)a.bins[1];
  hipError_t e = hipMemsetAsync(&a.work->counted2, 0, 2 * sizeof(u64), st);   // counted2, outside2
  if (e == hipSuccess) e = hipMemsetAsync(&a.work->cells[0], 0, cells * sizeof(u64), st);
  if (e != hipSuccess) return (int)e;
  if (cells <= ERPL_DIST_TILE_CELLS)
    hipLaunchKernelGGL(erpl_dist_hist2d<true>, dim3(grid_of(a.n)), dim3(ERPL_ANA_BLOCK), 0, st, a);
  else
    hipLaunchKernelGGL(erpl_dist_hist2d<false>, dim3(grid_of(a.n)), dim3(ERPL_ANA_BLOCK), 0, st, a);
  return (int)hipGetLastError();
}

int erpl_launch_dispersion(const ErplDispArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);
  hipLaunchKernelGGL(erpl_disp_moments<false>, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(erpl_disp_finish<false>, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a, nb);
  hipLaunchKernelGGL(erpl_disp_moments<true>, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(erpl_disp_finish<true>, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a, nb);
  hipLaunchKernelGGL(erpl_disp_inside, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(erpl_disp_finish_inside, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a, nb);
  return (int)hipGetLastError();
}
