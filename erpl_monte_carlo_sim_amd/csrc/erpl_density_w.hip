// erpl_density_w.hip — the device passes of erpl_mc_impact_density_weighted: the impact probability map of a flown run under
// another law, every sample with the integer weight erpl_mc_reweight gave it.  The passes are those of erpl_density.hip;
// whiten, nodes, fold, peak and fill_nan ARE its launchers (on the ErplDensWork inside ErplDensWWork), and so is the pair
// kernel (erpl_launch_densw_pairs: the weighted instantiation of erpl_dens_pairs).  The rest is here:
//
//   population  one streaming pass: the byte of every sample (0 = counted: mask byte 0, both rows finite, W > 0), the counts
//               in the order of the header, sum W and max W over the counted samples and the lowest column whose weight is
//               outside 0 .. 2^Q; its finish settles K (the bit length of max W) and S_d = sum_w 2^-K
//   gather      the counted points and their scaled weights w = W 2^-K (exact), in sample order, into dense arrays
//   moments     two passes over the dense arrays on the grid of the count: sum w x, sum w y, sum w w and the extremes, then
//               sum w (dx dx), w (dx dy), w (dy dy) about the mean read on the device
//   zones       over the dense points before they are whitened: per polygon sum W (integers: W = w 2^K, exact) and sum w w
//   regions     the radix selection of erpl_stat_device.h in its global-bin form over the f_j, sample j counting W_j times
//               (64-bit bins in LDS flushed to 64-bit global bins, a scan kernel between the passes), then one pass for
//               sum W [f >= t_k], min f and max f
// The order of every floating-point sum is fixed (erpl_stat_device.h; erpl_dens_slices for the pairs); the integer sums
// commute.  Integer atomics only (the histograms).  Compiled with -ffp-contract=off: every product of a sum rounds once.
#include "erpl_stat_device.h"
#include "erpl_reweight.h"

namespace {
constexpr int kL = ERPL_DENSITY_MAX_LEVELS, kZ = ERPL_DENSITY_MAX_ZONES;

struct DwTargets {   // by value into the selection's first kernel
  u64 rank[kL];
  int32_t n_levels;
};

// ---- population
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_population(const ErplDensWArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.row_x * n;
  const double* __restrict__ y = a.summary + (int64_t)a.row_y * n;
  const uint8_t* __restrict__ mask = a.mask;
  const int64_t* __restrict__ wt = a.weights;
  const int64_t most = (int64_t)1 << a.Q;
  u64 cnt[4] = {0ull, 0ull, 0ull, 0ull}, sum_w = 0ull;
  double max_w = 0.0, bad = INFINITY;
  // the loop bound is uniform over the wave: every lane takes part in every ballot
  for (int64_t base = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    int state = -1;
    if (i < n) {
      const int64_t W = wt[i];
      const bool admitted = W >= 0 && W <= most;
      if (!admitted && (double)i < bad) bad = (double)i;   // exact: i < 2^31
      if (mask && mask[i] != 0) state = 0;
      else if (!(finite_bits(x[i]) && finite_bits(y[i]))) state = 1;
      else if (W == 0 || !admitted) state = 2;
      else {
        state = 3;
        const double wd = (double)W;                       // exact: W <= 2^52
        sum_w += (u64)W;
        max_w = wd > max_w ? wd : max_w;
      }
      a.pop[i] = state == 3 ? 0 : 1;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] += (u64)__popcll(__ballot(state == k));
  }
  block_fold<Add, Max, Min>(sum_w, max_w, bad);
  const u64 s = counters_fold(cnt);
  ErplDensWWork* w = a.work;
  if (threadIdx.x == 0) { w->psum_w[blockIdx.x] = sum_w; w->pmax_w[blockIdx.x] = max_w; w->pbad[blockIdx.x] = bad; }
  if (threadIdx.x < 4) w->pcnt[blockIdx.x][threadIdx.x] = s;
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_finish_population(ErplDensWWork* w, const int nb) {
  u64 c0 = thread_partials<Add>(&w->pcnt[0][0], nb, 4), c1 = thread_partials<Add>(&w->pcnt[0][1], nb, 4);
  u64 c2 = thread_partials<Add>(&w->pcnt[0][2], nb, 4), c3 = thread_partials<Add>(&w->pcnt[0][3], nb, 4);
  u64 sum_w = thread_partials<Add>(w->psum_w, nb);
  double max_w = thread_partials<Max>(w->pmax_w, nb), bad = thread_partials<Min>(w->pbad, nb);
  block_fold<Add, Add, Add, Add, Add, Max, Min>(c0, c1, c2, c3, sum_w, max_w, bad);
  if (threadIdx.x == 0) {
    ErplDensWMoments& m = w->mom;
    const u64 mw = max_w > 0.0 ? (u64)max_w : 0ull;
    m.n_masked = c0; m.n_non_finite = c1; m.n_zero = c2; m.count = c3;
    m.sum_w = sum_w; m.max_w = mw; m.first_bad = bad;
    m.K = mw ? 64 - __clzll((long long)mw) : 0;
    m.reserved = 0;
    m.s_d = ldexp((double)sum_w, -m.K);
  }
}

// the counted points and their scaled weights, in sample order: xy[d], ws[d] of sample src[d], d < *count
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_gather(const ErplDensWArgs a, const uint32_t* __restrict__ src,
                                                            const u64* __restrict__ count, double2* __restrict__ xy,
                                                            double* __restrict__ ws) {
  const int64_t n = a.n, m = (int64_t)*count, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.row_x * n;
  const double* __restrict__ y = a.summary + (int64_t)a.row_y * n;
  const int K = a.work->mom.K;
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m && d < n; d += stride) {
    const uint32_t i = src[d];   // below n: the select wrote sample indices
    xy[d] = make_double2(x[i], y[i]);
    ws[d] = ldexp((double)a.weights[i], -K);
  }
}

// ---- moments over the dense arrays, on the grid of m = *count (the launch has the grid of n; the workgroups beyond leave).
// SECOND = false: sum w x, sum w y, sum w w and the extremes; SECOND = true: sum w (dx dx), w (dx dy), w (dy dy).
template <bool SECOND>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_moments(ErplDensWWork* w, const u64* __restrict__ count,
                                                             const double2* __restrict__ xy, const double* __restrict__ ws) {
  const int64_t m = (int64_t)*count;
  const int nb = grid_of(m);
  if ((int)blockIdx.x >= nb) return;
  const int64_t stride = (int64_t)nb * ERPL_ANA_BLOCK;
  const double mx = SECOND ? w->mom.mean_x : 0.0, my = SECOND ? w->mom.mean_y : 0.0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  double lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m; d += stride) {
    const double2 p = xy[d];
    const double wd = ws[d];
    if (SECOND) {
      const double dx = p.x - mx, dy = p.y - my;
      s0 += wd * (dx * dx); s1 += wd * (dx * dy); s2 += wd * (dy * dy);
    } else {
      s0 += wd * p.x; s1 += wd * p.y; s2 += wd * wd;
      lox = p.x < lox ? p.x : lox; hix = p.x > hix ? p.x : hix;
      loy = p.y < loy ? p.y : loy; hiy = p.y > hiy ? p.y : hiy;
    }
  }
  block_fold<Add, Add, Add>(s0, s1, s2);
  if (!SECOND) block_fold<Min, Max, Min, Max>(lox, hix, loy, hiy);
  if (threadIdx.x == 0) {
    ErplDensWork& d = w->d;
    d.psum[0][blockIdx.x] = s0; d.psum[1][blockIdx.x] = s1; d.psum[2][blockIdx.x] = s2;
    if (!SECOND) {
      d.pext[0][blockIdx.x] = lox; d.pext[1][blockIdx.x] = hix;
      d.pext[2][blockIdx.x] = loy; d.pext[3][blockIdx.x] = hiy;
    }
  }
}

template <bool SECOND>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_finish_moments(ErplDensWWork* w, const u64* __restrict__ count) {
  const int nb = grid_of((int64_t)*count);
  const ErplDensWork& d = w->d;
  double s0 = thread_partials<Add>(d.psum[0], nb), s1 = thread_partials<Add>(d.psum[1], nb), s2 = thread_partials<Add>(d.psum[2], nb);
  block_fold<Add, Add, Add>(s0, s1, s2);
  ErplDensWMoments& m = w->mom;
  if (SECOND) {
    if (threadIdx.x == 0) { m.sxx = s0; m.sxy = s1; m.syy = s2; }
    return;
  }
  double lox = thread_partials<Min>(d.pext[0], nb), hix = thread_partials<Max>(d.pext[1], nb);
  double loy = thread_partials<Min>(d.pext[2], nb), hiy = thread_partials<Max>(d.pext[3], nb);
  block_fold<Min, Max, Min, Max>(lox, hix, loy, hiy);
  if (threadIdx.x == 0) {
    m.mean_x = s0 / m.s_d;   // NaN for an empty cloud; the host reports it as NaN
    m.mean_y = s1 / m.s_d;
    m.sum_w2 = s2;
    m.min_x = lox; m.max_x = hix; m.min_y = loy; m.max_y = hiy;
  }
}

// ---- zones: per polygon the weight inside, over the dense points (m >= 1; W = w 2^K, exact)
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_zones(ErplDensWWork* w, const int n_zones, const double2* __restrict__ xy,
                                                           const double* __restrict__ ws, const int64_t m) {
  __shared__ double s_vx[ERPL_DENSITY_MAX_VERTICES], s_vy[ERPL_DENSITY_MAX_VERTICES];
  __shared__ int s_first[kZ + 1];
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double unit = ldexp(1.0, w->mom.K);
  for (int k = threadIdx.x; k < ERPL_DENSITY_MAX_VERTICES; k += ERPL_ANA_BLOCK) {
    s_vx[k] = w->d.in.zone_x[k];
    s_vy[k] = w->d.in.zone_y[k];
  }
  if (threadIdx.x <= kZ) s_first[threadIdx.x] = w->d.in.zone_first[threadIdx.x];
  __syncthreads();
  u64 in[kZ];
  double a2[kZ];
#pragma unroll
  for (int z = 0; z < kZ; ++z) { in[z] = 0ull; a2[z] = 0.0; }
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m; d += stride) {
    const double2 p = xy[d];
    const double wd = ws[d];
    const u64 W = (u64)(wd * unit);
    const double w2 = wd * wd;
#pragma unroll
    for (int z = 0; z < kZ; ++z) {
      if (z >= n_zones) continue;
      const int v0 = s_first[z], v1 = s_first[z + 1];   // the host has checked 0 <= v0, v0 + 3 <= v1 <= 256
      bool c = false;
      for (int vi = v0, vj = v1 - 1; vi < v1; vj = vi++)
        if (erpl_zone_flips(p.x, p.y, s_vx[vi], s_vy[vi], s_vx[vj], s_vy[vj])) c = !c;   // THE crossing rule (erpl_tally.h)
      if (c) { in[z] += W; a2[z] += w2; }
    }
  }
#pragma unroll
  for (int z = 0; z < kZ; ++z) {
    if (z >= n_zones) break;   // uniform over the workgroup
    block_fold_again<Add, Add>(in[z], a2[z]);
    if (threadIdx.x == 0) { w->d.zpart[blockIdx.x][z] = in[z]; w->za2[blockIdx.x][z] = a2[z]; }
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_finish_zones(ErplDensWWork* w, const int n_zones, const int nb) {
  for (int z = 0; z < n_zones; ++z) {
    u64 s = thread_partials<Add>(&w->d.zpart[0][z], nb, kZ);
    double a2 = thread_partials<Add>(&w->za2[0][z], nb, kZ);
    block_fold_again<Add, Add>(s, a2);   // the same scratch in every round
    if (threadIdx.x == 0) { w->out.zone_w[z] = s; w->out.zone_a2[z] = a2; }
  }
}

// ---- regions: the weighted selection over the f_j (erpl_stat_device.h, global bins)

// every target in one group (no digit is fixed yet), its rank from the host, the histograms empty
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_select_init(ErplDensWWork* w, const DwTargets t) {
  if (threadIdx.x < kL) select_start(w->sel, w->out.key, threadIdx.x, (int)threadIdx.x < t.n_levels ? t.rank[threadIdx.x] : 0ull);
  select_clear<ERPL_ANA_BLOCK>(&w->hist[0][0], kL * ERPL_ANA_BINS);
}

// a digit pass over the row: a counted sample of non-zero weight counts W times
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_hist(const ErplDensWArgs a, const double* __restrict__ row, const int n_levels,
                                                          const int shift) {
  const int64_t* __restrict__ wt = a.weights;
  const uint8_t* __restrict__ pop = a.pop;
  select_pass<u64>(a.work->sel, a.work->hist, n_levels, a.n, shift, [=](int64_t i, u64* key, u64* w) {
    if (pop[i] != 0) return false;
    *w = (u64)wt[i];
    *key = key_of_signed(row[i]);
    return *w != 0ull;
  });
}

__global__ __launch_bounds__(64 * kL) void dw_scan(ErplDensWWork* w, const int n_levels, const int shift) {
  select_step(w->sel, w->hist, w->out.key, n_levels, shift);
}

// the weight at or above every threshold, and the extremes of the f_j
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_content(const ErplDensWArgs a, const double* __restrict__ row, const int n_levels) {
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const int64_t* __restrict__ wt = a.weights;
  const uint8_t* __restrict__ pop = a.pop;
  ErplDensWWork* w = a.work;
  double thr[kL];
  u64 c[kL];
#pragma unroll
  for (int k = 0; k < kL; ++k) { thr[k] = erpl_double_of(erpl_tally_bits_of_key(w->out.key[k])); c[k] = 0ull; }
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < n; i += stride) {
    if (pop[i] != 0) continue;
    const double f = row[i];
    const u64 W = (u64)wt[i];
    mn = f < mn ? f : mn;
    mx = f > mx ? f : mx;
#pragma unroll
    for (int k = 0; k < kL; ++k)
      if (k < n_levels && f >= thr[k]) c[k] += W;
  }
  block_fold<Min, Max>(mn, mx);
  if (threadIdx.x == 0) { w->d.pext[0][blockIdx.x] = mn; w->d.pext[1][blockIdx.x] = mx; }
#pragma unroll
  for (int k = 0; k < kL; ++k) {
    if (k >= n_levels) break;   // uniform over the workgroup
    block_fold_again<Add>(c[k]);
    if (threadIdx.x == 0) w->cpart[blockIdx.x][k] = c[k];
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void dw_finish_content(ErplDensWWork* w, const int n_levels, const int nb) {
  double mn = thread_partials<Min>(w->d.pext[0], nb), mx = thread_partials<Max>(w->d.pext[1], nb);
  block_fold<Min, Max>(mn, mx);
  if (threadIdx.x == 0) { w->out.f_min = mn; w->out.f_max = mx; }
  for (int k = 0; k < n_levels; ++k) {
    u64 c = thread_partials<Add>(&w->cpart[0][k], nb, kL);
    block_fold_again<Add>(c);
    if (threadIdx.x == 0) w->out.content_w[k] = c;
  }
}

}  // namespace

int erpl_launch_densw_population(const ErplDensWArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);
  hipLaunchKernelGGL(dw_population, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(dw_finish_population, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, nb);
  return (int)hipGetLastError();
}

int erpl_launch_densw_moments(const ErplDensWArgs& a, const uint32_t* src, const unsigned long long* count, double* xy, double* ws,
                              void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);   // of n: the count is on the device; the kernels keep to the grid of the count
  double2* p = (double2*)xy;
  hipLaunchKernelGGL(dw_gather, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a, src, count, p, ws);
  hipLaunchKernelGGL(dw_moments<false>, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a.work, count, p, ws);
  hipLaunchKernelGGL(dw_finish_moments<false>, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, count);
  hipLaunchKernelGGL(dw_moments<true>, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a.work, count, p, ws);
  hipLaunchKernelGGL(dw_finish_moments<true>, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, count);
  return (int)hipGetLastError();
}

int erpl_launch_densw_zones(const ErplDensWArgs& a, const double* xy, const double* ws, int64_t m, void* stream) {
  if (m <= 0 || a.n_zones <= 0) return 0;   // the host has cleared work->out
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(m);
  hipLaunchKernelGGL(dw_zones, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a.work, a.n_zones, (const double2*)xy, ws, m);
  hipLaunchKernelGGL(dw_finish_zones, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, a.n_zones, nb);
  return (int)hipGetLastError();
}

int erpl_launch_densw_regions(const ErplDensWArgs& a, const double* row, const unsigned long long* rank, int n_levels, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);
  DwTargets t = {};
  t.n_levels = n_levels;
  for (int k = 0; k < n_levels; ++k) t.rank[k] = rank[k];
  hipLaunchKernelGGL(dw_select_init, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, t);
  if (n_levels > 0)
    for (int shift = 56; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(dw_hist, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a, row, n_levels, shift);
      hipLaunchKernelGGL(dw_scan, dim3(1), dim3(64 * kL), 0, st, a.work, n_levels, shift);
    }
  hipLaunchKernelGGL(dw_content, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a, row, n_levels);
  hipLaunchKernelGGL(dw_finish_content, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, n_levels, nb);
  return (int)hipGetLastError();
}
