// erpl_density.hip — the device passes of erpl_mc_impact_density: the impact probability map.  A Gaussian kernel density
// estimate of the landing points at the nodes of a grid and at the points themselves, and the landings inside polygons;
// the thresholds of the highest-density regions come from erpl_launch_row_stats (erpl_analysis.hip) on the sample row.
//
//   compact   the population bytes (0 = counted), rocPRIM's select on them (erpl_launch_boot_compact) and the gather of the
//             counted points, in sample order, into a dense array
//   moments   two passes over the DENSE points in the pattern of erpl_distributions.hip (sums, then the sums about the mean
//             read on the device), min / max riding on the first, on the grid of the count: what lies between the counted
//             samples does not reach a sum
//   whiten    the dense points, in place, and the nodes: centred and mapped through the inverse Cholesky factor of H; the
//             pair exponent is then -(du du + dv dv) / 2
//   pairs     THE hot loop, all pairs, fp64, compute-bound: sum_i exp(-|q - s_i|^2 / 2) for an arbitrary list of query
//             points, launched once over the nodes and once over the dense points themselves.  A workgroup owns
//             ERPL_DENS_TILE queries - ERPL_DENS_Q per thread, independent exp chains side by side - and one slice of the
//             sources, staged through a 16 KB LDS tile and read back at one address per wave (a broadcast).  Per pair two
//             subtractions, one product, one explicit FMA (the unit is built without contraction), one product by -0.5,
//             ocml's exp and one addition.  The weighted map (erpl_density_w.hip) runs the same kernel with a weight per
//             source: a 24 KB tile, and an explicit FMA in the place of the addition.
//   fold      the slices of a query added in slice order, times the normalisation; the sample pass scatters to the row
//   zones     one streaming pass: the even-odd crossing rule against the vertices (staged in LDS), ballots and popcounts
//   peak      sum and maximum of the nodes, then the first node that holds the maximum, by fixed-order folds
// The order of every sum is fixed (erpl_stat_device.h; erpl_dens_slices in erpl_tables.h for the pairs): a thread adds
// its sources in index order, slices are added in slice order.  No floating-point atomics.  Compiled with
// -ffp-contract=off: the crossing expression is rounded as NumPy rounds it.
#include "erpl_stat_device.h"
#include "erpl_tally.h"

namespace {

// ---- population: the byte of every sample (0 = counted) that rocPRIM's select turns into the dense population
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_population(const ErplDensArgs a) {
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.row_x * n;
  const double* __restrict__ y = a.summary + (int64_t)a.row_y * n;
  const uint8_t* __restrict__ mask = a.mask;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < n; i += stride)
    a.pop[i] = finite_bits(x[i]) && finite_bits(y[i]) && (!mask || mask[i] == 0) ? 0 : 1;
}

// the counted points, in sample order: xy[d] = (x, y) of sample src[d], d < *count
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_gather(const ErplDensArgs a, const uint32_t* __restrict__ src,
                                                                   const u64* __restrict__ count, double2* __restrict__ xy) {
  const int64_t n = a.n, m = (int64_t)*count, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.row_x * n;
  const double* __restrict__ y = a.summary + (int64_t)a.row_y * n;
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m && d < n; d += stride) {
    const uint32_t i = src[d];   // below n: the select wrote sample indices
    xy[d] = make_double2(x[i], y[i]);
  }
}

// ---- moments over the DENSE points, on the grid of m = *count (the launch has the grid of n; the workgroups beyond leave):
// the sums depend on the counted samples in their order alone, not on what lies between them.  SECOND = false: sums and
// extremes of x and y; SECOND = true: sums of dx dx, dx dy, dy dy about the mean of the first pass.
template <bool SECOND>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_moments(ErplDensWork* w, const u64* __restrict__ count,
                                                                    const double2* __restrict__ xy) {
  const int64_t m = (int64_t)*count;
  const int nb = grid_of(m);
  if ((int)blockIdx.x >= nb) return;
  const int64_t stride = (int64_t)nb * ERPL_ANA_BLOCK;
  const double mx = SECOND ? w->mom.mean_x : 0.0, my = SECOND ? w->mom.mean_y : 0.0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  double lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m; d += stride) {
    const double2 p = xy[d];
    if (SECOND) {
      const double dx = p.x - mx, dy = p.y - my;
      s0 += dx * dx; s1 += dx * dy; s2 += dy * dy;
    } else {
      s0 += p.x; s1 += p.y;
      lox = p.x < lox ? p.x : lox; hix = p.x > hix ? p.x : hix;
      loy = p.y < loy ? p.y : loy; hiy = p.y > hiy ? p.y : hiy;
    }
  }
  if (SECOND) {
    block_fold<Add, Add, Add>(s0, s1, s2);
  } else {
    block_fold<Add, Add>(s0, s1);
    block_fold<Min, Max, Min, Max>(lox, hix, loy, hiy);
  }
  if (threadIdx.x == 0) {
    w->psum[0][blockIdx.x] = s0;
    w->psum[1][blockIdx.x] = s1;
    if (SECOND) {
      w->psum[2][blockIdx.x] = s2;
    } else {
      w->pext[0][blockIdx.x] = lox; w->pext[1][blockIdx.x] = hix;
      w->pext[2][blockIdx.x] = loy; w->pext[3][blockIdx.x] = hiy;
    }
  }
}

template <bool SECOND>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_finish_moments(ErplDensWork* w, const u64* __restrict__ count) {
  const u64 cnt = *count;
  const int nb = grid_of((int64_t)cnt);
  double s0 = thread_partials<Add>(w->psum[0], nb), s1 = thread_partials<Add>(w->psum[1], nb);
  ErplDensMoments& m = w->mom;
  if (SECOND) {
    double s2 = thread_partials<Add>(w->psum[2], nb);
    block_fold<Add, Add, Add>(s0, s1, s2);
    if (threadIdx.x == 0) { m.sxx = s0; m.sxy = s1; m.syy = s2; }
    return;
  }
  double lox = thread_partials<Min>(w->pext[0], nb), hix = thread_partials<Max>(w->pext[1], nb);
  double loy = thread_partials<Min>(w->pext[2], nb), hiy = thread_partials<Max>(w->pext[3], nb);
  block_fold<Add, Add>(s0, s1);
  block_fold<Min, Max, Min, Max>(lox, hix, loy, hiy);
  if (threadIdx.x == 0) {
    m.count = cnt;
    m.mean_x = s0 / (double)cnt;   // NaN for an empty cloud; the host reports it as NaN
    m.mean_y = s1 / (double)cnt;
    m.min_x = lox; m.max_x = hix; m.min_y = loy; m.max_y = hiy;
  }
}

// ---- whitened coordinates
__device__ __forceinline__ void dens_map(const ErplDensMap& t, double px, double py, double& u, double& v) {
  const double dx = px - t.mean_x, dy = py - t.mean_y;
  u = t.w11 * dx;
  v = __builtin_fma(t.w21, dx, t.w22 * dy);
}

// the dense points, in place
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_whiten(double2* __restrict__ xy, const int64_t m, const ErplDensMap t) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t d = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; d < m; d += stride) {
    const double2 p = xy[d];
    double u, v;
    dens_map(t, p.x, p.y, u, v);
    xy[d] = make_double2(u, v);
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_nodes(const ErplDensWork* __restrict__ w, const int nx, const int ny,
                                                                  const ErplDensMap t, double2* __restrict__ uv) {
  const int64_t nodes = (int64_t)nx * ny, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t q = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; q < nodes; q += stride) {
    double u, v;
    dens_map(t, w->in.grid_x[q / ny], w->in.grid_y[q % ny], u, v);
    uv[q] = make_double2(u, v);
  }
}

// ---- pairs: workgroup (bx, by) adds the sources by * per_slice .. min(m, (by + 1) * per_slice) - 1, in index order, for
// the queries bx * ERPL_DENS_TILE + k * ERPL_ANA_BLOCK + thread, k < ERPL_DENS_Q, into partial[by][query].
// WEIGHTED (erpl_mc_impact_density_weighted): source j counts ws[j] times - its weight rides in the LDS tile, (u, v, w) and
// 24 KB, and the addition becomes one explicit FMA, acc = fma(w, exp(-0.5 e), acc).  Otherwise ws is not looked at.
template <bool WEIGHTED>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_pairs(const double2* __restrict__ qry, const int64_t nq,
                                                                  const double2* __restrict__ src, const double* __restrict__ ws,
                                                                  const int64_t m, const int64_t per_slice,
                                                                  double* __restrict__ partial) {
  __shared__ double2 s_src[ERPL_DENS_TILE];
  __shared__ double s_w[WEIGHTED ? ERPL_DENS_TILE : 1];   // (unused, and gone, without weights)
  const int tid = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * ERPL_DENS_TILE + tid;
  const int64_t first = (int64_t)blockIdx.y * per_slice;
  const int64_t last = first + per_slice < m ? first + per_slice : m;
  double qu[ERPL_DENS_Q], qv[ERPL_DENS_Q], acc[ERPL_DENS_Q];
#pragma unroll
  for (int k = 0; k < ERPL_DENS_Q; ++k) {
    const int64_t q = q0 + (int64_t)k * ERPL_ANA_BLOCK;
    const double2 p = q < nq ? qry[q] : make_double2(0.0, 0.0);   // a lane without a query computes and stores nothing
    qu[k] = p.x; qv[k] = p.y; acc[k] = 0.0;
  }
  for (int64_t base = first; base < last; base += ERPL_DENS_TILE) {
    const int cnt = (int)(last - base < ERPL_DENS_TILE ? last - base : ERPL_DENS_TILE);
    __syncthreads();   // the tile before has been read
    for (int j = tid; j < cnt; j += ERPL_ANA_BLOCK) {
      s_src[j] = src[base + j];
      if (WEIGHTED) s_w[j] = ws[base + j];
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const double2 s = s_src[j];   // one address per wave: a broadcast
      const double wj = WEIGHTED ? s_w[j] : 1.0;
#pragma unroll
      for (int k = 0; k < ERPL_DENS_Q; ++k) {
        const double du = qu[k] - s.x, dv = qv[k] - s.y;
        const double e = __builtin_fma(dv, dv, du * du);
        if (WEIGHTED) acc[k] = __builtin_fma(wj, exp(-0.5 * e), acc[k]);
        else acc[k] += exp(-0.5 * e);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ERPL_DENS_Q; ++k) {
    const int64_t q = q0 + (int64_t)k * ERPL_ANA_BLOCK;
    if (q < nq) partial[(int64_t)blockIdx.y * nq + q] = acc[k];
  }
}

// the slices of a query in slice order, normalised; scatter: the sample of dense query q (the row of the sample pass)
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_fold(const double* __restrict__ partial, const int slices,
                                                                 const int64_t nq, const double norm, double* __restrict__ out,
                                                                 const uint32_t* __restrict__ scatter) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t q = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; q < nq; q += stride) {
    double s = partial[q];
    for (int k = 1; k < slices; ++k) s += partial[(int64_t)k * nq + q];
    out[scatter ? (int64_t)scatter[q] : q] = norm * s;
  }
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_fill_nan(double* __restrict__ row, const int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; i < n; i += stride) row[i] = NAN;
}

// ---- zones: the counted samples inside every polygon
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_zones(const ErplDensArgs a) {
  __shared__ double s_vx[ERPL_DENSITY_MAX_VERTICES], s_vy[ERPL_DENSITY_MAX_VERTICES];
  __shared__ int s_first[ERPL_DENSITY_MAX_ZONES + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = a.n, stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double* __restrict__ x = a.summary + (int64_t)a.row_x * n;
  const double* __restrict__ y = a.summary + (int64_t)a.row_y * n;
  const uint8_t* __restrict__ pop = a.pop;
  for (int k = threadIdx.x; k < ERPL_DENSITY_MAX_VERTICES; k += ERPL_ANA_BLOCK) {
    s_vx[k] = a.work->in.zone_x[k];
    s_vy[k] = a.work->in.zone_y[k];
  }
  if (threadIdx.x <= ERPL_DENSITY_MAX_ZONES) s_first[threadIdx.x] = a.work->in.zone_first[threadIdx.x];
  __syncthreads();
  u64 in[ERPL_DENSITY_MAX_ZONES];
#pragma unroll
  for (int z = 0; z < ERPL_DENSITY_MAX_ZONES; ++z) in[z] = 0ull;
  for (int64_t base = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    const bool use = i < n && pop[i] == 0;
    const double px = use ? x[i] : 0.0, py = use ? y[i] : 0.0;
#pragma unroll
    for (int z = 0; z < ERPL_DENSITY_MAX_ZONES; ++z) {
      if (z >= a.n_zones) continue;
      const int v0 = s_first[z], v1 = s_first[z + 1];   // the host has checked 0 <= v0, v0 + 3 <= v1 <= 256
      bool c = false;
      for (int vi = v0, vj = v1 - 1; vi < v1; vj = vi++) {
        const double xi = s_vx[vi], yi = s_vy[vi], xj = s_vx[vj], yj = s_vy[vj];
        if (erpl_zone_flips(px, py, xi, yi, xj, yj)) c = !c;   // the one definition of the crossing rule (erpl_tally.h)
      }
      in[z] += __popcll(__ballot(use && c));
    }
  }
  const u64 s = counters_fold(in);
  if (threadIdx.x < ERPL_DENSITY_MAX_ZONES) a.work->zpart[blockIdx.x][threadIdx.x] = s;
}

__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_finish_zones(ErplDensWork* w, const int nb) {
  for (int z = 0; z < ERPL_DENSITY_MAX_ZONES; ++z) {
    u64 s = thread_partials<Add>(&w->zpart[0][z], nb, ERPL_DENSITY_MAX_ZONES);
    block_fold_again<Add>(s);   // the same scratch in every round
    if (threadIdx.x == 0) w->out.zone_inside[z] = s;
  }
}

// ---- peak.  AT = false: sum and maximum of the node values; AT = true: the first node that holds the maximum (its index
// as a double: exact, there are at most 2^18 nodes).
template <bool AT>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_peak(ErplDensWork* w, const double* __restrict__ f, const int64_t nodes) {
  const int64_t stride = (int64_t)gridDim.x * ERPL_ANA_BLOCK;
  const double peak = AT ? w->out.peak : 0.0;
  double s = 0.0, mx = -INFINITY, at = INFINITY;
  for (int64_t q = (int64_t)blockIdx.x * ERPL_ANA_BLOCK + threadIdx.x; q < nodes; q += stride) {
    const double v = f[q];
    if (AT) {
      if (v == peak && (double)q < at) at = (double)q;
    } else {
      s += v;
      mx = v > mx ? v : mx;
    }
  }
  if (AT) {
    block_fold<Min>(at);
    if (threadIdx.x == 0) w->pext[0][blockIdx.x] = at;
  } else {
    block_fold<Add, Max>(s, mx);
    if (threadIdx.x == 0) { w->psum[0][blockIdx.x] = s; w->pext[0][blockIdx.x] = mx; }
  }
}

template <bool AT>
__global__ __launch_bounds__(ERPL_ANA_BLOCK) void erpl_dens_finish_peak(ErplDensWork* w, const int nb) {
  if (AT) {
    double at = thread_partials<Min>(w->pext[0], nb);
    block_fold<Min>(at);
    if (threadIdx.x == 0) w->out.peak_at = at;
  } else {
    double s = thread_partials<Add>(w->psum[0], nb), mx = thread_partials<Max>(w->pext[0], nb);
    block_fold<Add, Max>(s, mx);
    if (threadIdx.x == 0) { w->out.sum = s; w->out.peak = mx; }
  }
}

}  // namespace

int erpl_launch_dens_population(const ErplDensArgs& a, void* stream) {
  hipLaunchKernelGGL(erpl_dens_population, dim3(grid_of(a.n)), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int erpl_launch_dens_moments(const ErplDensArgs& a, const uint32_t* src, const unsigned long long* count, double* xy,
                             void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);   // of n: the count is on the device; the kernels keep to the grid of the count
  double2* p = (double2*)xy;
  hipLaunchKernelGGL(erpl_dens_gather, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a, src, count, p);
  hipLaunchKernelGGL(erpl_dens_moments<false>, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a.work, count, p);
  hipLaunchKernelGGL(erpl_dens_finish_moments<false>, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, count);
  hipLaunchKernelGGL(erpl_dens_moments<true>, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a.work, count, p);
  hipLaunchKernelGGL(erpl_dens_finish_moments<true>, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, count);
  return (int)hipGetLastError();
}

int erpl_launch_dens_zones(const ErplDensArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(a.n);
  hipLaunchKernelGGL(erpl_dens_zones, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(erpl_dens_finish_zones, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, a.work, nb);
  return (int)hipGetLastError();
}

int erpl_launch_dens_whiten(double* xy, int64_t m, const ErplDensMap& map, void* stream) {
  hipLaunchKernelGGL(erpl_dens_whiten, dim3(grid_of(m)), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, (double2*)xy, m, map);
  return (int)hipGetLastError();
}

int erpl_launch_dens_nodes(const ErplDensWork* work, int nx, int ny, const ErplDensMap& map, double* uv, void* stream) {
  hipLaunchKernelGGL(erpl_dens_nodes, dim3(grid_of((int64_t)nx * ny)), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, work, nx,
                     ny, map, (double2*)uv);
  return (int)hipGetLastError();
}

// the pair kernel over the slices of erpl_dens_slices; returns their number
template <bool WEIGHTED>
static int launch_pairs(const double* qry, int64_t queries, const double* src, const double* ws, int64_t m, double* partial,
                        hipStream_t st) {
  int64_t per_slice = 0;
  const int slices = erpl_dens_slices(m, queries, &per_slice);
  const int64_t blocks = (queries + ERPL_DENS_TILE - 1) / ERPL_DENS_TILE;
  hipLaunchKernelGGL(erpl_dens_pairs<WEIGHTED>, dim3((unsigned)blocks, (unsigned)slices), dim3(ERPL_ANA_BLOCK), 0, st,
                     (const double2*)qry, queries, (const double2*)src, ws, m, per_slice, partial);
  return slices;
}

int erpl_launch_dens_pairs(const double* qry, int64_t queries, const double* src, int64_t m, double norm, double* partial,
                           double* out, const uint32_t* scatter, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int slices = launch_pairs<false>(qry, queries, src, nullptr, m, partial, st);
  hipLaunchKernelGGL(erpl_dens_fold, dim3(grid_of(queries)), dim3(ERPL_ANA_BLOCK), 0, st, partial, slices, queries, norm, out,
                     scatter);
  return (int)hipGetLastError();
}

int erpl_launch_densw_pairs(const double* qry, int64_t queries, const double* src, const double* ws, int64_t m, double* partial,
                            void* stream) {
  launch_pairs<true>(qry, queries, src, ws, m, partial, (hipStream_t)stream);
  return (int)hipGetLastError();
}

int erpl_launch_dens_fold(const double* partial, int slices, int64_t queries, double norm, double* out, const uint32_t* scatter,
                          void* stream) {
  hipLaunchKernelGGL(erpl_dens_fold, dim3(grid_of(queries)), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, partial, slices,
                     queries, norm, out, scatter);
  return (int)hipGetLastError();
}

int erpl_launch_dens_peak(ErplDensWork* work, const double* density, int64_t nodes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(nodes);
  hipLaunchKernelGGL(erpl_dens_peak<false>, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, work, density, nodes);
  hipLaunchKernelGGL(erpl_dens_finish_peak<false>, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, work, nb);
  hipLaunchKernelGGL(erpl_dens_peak<true>, dim3(nb), dim3(ERPL_ANA_BLOCK), 0, st, work, density, nodes);
  hipLaunchKernelGGL(erpl_dens_finish_peak<true>, dim3(1), dim3(ERPL_ANA_BLOCK), 0, st, work, nb);
  return (int)hipGetLastError();
}

int erpl_launch_dens_fill_nan(double* row, int64_t n, void* stream) {
  hipLaunchKernelGGL(erpl_dens_fill_nan, dim3(grid_of(n)), dim3(ERPL_ANA_BLOCK), 0, (hipStream_t)stream, row, n);
  return (int)hipGetLastError();
}
