// erpl_casualty.hip — erpl_mc_casualty (include/erpl_mc.h): the casualty expectation of a debris footprint, its hazard map in
// exact integers and the smoothed individual-risk map.  Device passes and the host half in one unit, as erpl_reweight.hip.
//
//   population  the raster checked once: entries that are negative or not finite are counted, the call is refused before
//               anything else runs
//   traj        one lane per column, serially over (k, f): the trajectory's expectation e_j in the order of the header
//   totals      two passes over the row of the e_j in the pattern of erpl_density.hip (sum, maximum and count; then the
//               squares about the mean and the first column that holds the maximum), on the grid of m
//   rows        one workgroup per row r = (k, f), walking its columns as erpl_mc_corridor_bands walks a matrix: the counts,
//               S_kf (a thread adds its columns in index order, then the fixed-order fold), the integer adds of the hazard map
//               and the stable compaction of the lethal jobs, in column order, into the group's dense array
//   groups      one workgroup per row: mean and covariance from two fixed-order passes over the dense members, H, its
//               Cholesky factor and the normalisation by thread 0, then the members whitened in place
//   pairs       THE hot loop: a workgroup owns ERPL_CAS_TILE cell centres - ERPL_DENS_Q per thread - and one slice of the rows
//               (erpl_cas_slices); per row it maps its centres through the group's factor and adds the group's members, staged
//               through a 16 KB LDS tile and read back at one address per wave; the inner loop is erpl_density.hip's
//   fold        the slices of a cell added in slice order
// What is left - the split by node and fragment, the map in doubles, ec_map, ec_smooth, mix_mass, the level areas - is a walk
// over at most 2^20 cells and 4096 rows: the host does it in index order.  No floating-point atomics anywhere; the map takes
// integer atomics alone.  Compiled with -ffp-contract=off; the FMAs that are wanted are written out.
#include <stddef.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "erpl_stat_device.h"   // first: the HIP runtime, which erpl_tally.h expects
#include "erpl_casualty.h"
#include "erpl_host.h"

namespace {

constexpr int kBlock = ERPL_ANA_BLOCK;
constexpr int kTileEdge = 64;                      // the LDS tile in front of the map: kTileEdge x kTileEdge hit counts, 16 KB
constexpr int kMaxRows = ERPL_CORRIDOR_MAX_NODES;  // n_nodes * n_fragments

struct CasRow {        // what the row pass and the group pass leave per row
  u64 cnt[4];          // landed, lethal, off_grid, missing
  u64 n_use;           // the members the smoothing pass adds: cnt[1], or 0 for a group that is not solid
  double S, mean_x, mean_y, hxx, hxy, hyy;
  double w11, w21, w22, norm;
};
struct CasTotals {
  u64 m_c;
  double sum, mean, max, ss, col;
};
struct CasWork {
  unsigned int bad, pad;
  CasTotals tot;
  double psum[ERPL_ANA_MAX_BLOCKS], pext[ERPL_ANA_MAX_BLOCKS];
  u64 pcnt[ERPL_ANA_MAX_BLOCKS];
  double p_fail[kMaxRows], w[kMaxRows];
  long long W[kMaxRows];
  CasRow row[kMaxRows];
};

struct CasArgs {
  const double* values;
  const uint8_t* mask;
  const double* population;
  CasWork* work;
  unsigned long long* words;
  double* ec;
  double2* pts;
  int64_t m, ld;
  int32_t n_nodes, n_fragments, smooth, reserved;
  double ke_min, bw_scale, h_floor;
  ErplCasRaster g;
  double c_f[ERPL_DEBRIS_MAX_FRAGMENTS], half_mass[ERPL_DEBRIS_MAX_FRAGMENTS];
};

// ---- population: how many entries are negative or not finite
__global__ __launch_bounds__(kBlock) void cas_population(const double* __restrict__ pop, const int64_t cells, CasWork* w) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  unsigned int bad = 0u;
  for (int64_t base = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~63); base < cells; base += stride) {
    const int64_t c = base + (threadIdx.x & 63);
    const bool b = c < cells && !(finite_bits(pop[c]) && pop[c] >= 0.0);
    bad += (unsigned int)__popcll(__ballot(b));
  }
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&w->bad, bad);
}

// ---- traj: e_j of every column, NaN for a column that is not counted
__global__ __launch_bounds__(kBlock) void cas_traj(const CasArgs a) {
  const int64_t m = a.m, ld = a.ld, stride = (int64_t)gridDim.x * kBlock;
  const int K = a.n_nodes, F = a.n_fragments;
  const int64_t R = (int64_t)K * F;
  const ErplEdges ex = erpl_edges_of(a.g.lo_x, a.g.hi_x, a.g.bins_x), ey = erpl_edges_of(a.g.lo_y, a.g.hi_y, a.g.bins_y);
  const double* __restrict__ X = a.values + (int64_t)ERPL_IIP_CH_X * R * ld;
  const double* __restrict__ Y = a.values + (int64_t)ERPL_IIP_CH_Y * R * ld;
  const double* __restrict__ V = a.values + (int64_t)ERPL_IIP_CH_VIMPACT * R * ld;
  const double* __restrict__ pf = a.work->p_fail;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
    if (a.mask && a.mask[j] != 0) { a.ec[j] = NAN; continue; }
    double e = 0.0;
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
      for (int f = 0; f < F; ++f) {
        const int64_t at = ((int64_t)k * F + f) * ld + j;
        const double x = X[at], y = Y[at];
        int32_t cell = 0;
        double h = 0.0;
        if ((erpl_cas_class(x, y, V[at], a.half_mass[f], a.ke_min) & ERPL_CAS_LETHAL) && erpl_cas_cell(a.g, ex, ey, x, y, &cell))
          h = a.c_f[f] * a.population[cell];
        s += h;
      }
      e += pf[k] * s;
    }
    a.ec[j] = e;
  }
}

// ---- totals over the row of the e_j.  SECOND = false: sum, maximum and count of the counted columns; SECOND = true: the
// squares about the mean and the first column that holds the maximum (as a double: exact, m < 2^31).
template <bool SECOND>
__global__ __launch_bounds__(kBlock) void cas_totals(const CasArgs a) {
  const int64_t m = a.m, stride = (int64_t)gridDim.x * kBlock;
  const double mean = SECOND ? a.work->tot.mean : 0.0, top = SECOND ? a.work->tot.max : 0.0;
  double s = 0.0, mx = -INFINITY, col = INFINITY;
  u64 cnt = 0ull;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
    if (a.mask && a.mask[j] != 0) continue;
    const double e = a.ec[j];
    if (SECOND) {
      const double d = e - mean;
      s += d * d;
      if (e == top && (double)j < col) col = (double)j;
    } else {
      s += e;
      mx = e > mx ? e : mx;
      cnt += 1ull;
    }
  }
  if (SECOND) {
    block_fold<Add, Min>(s, col);
    if (threadIdx.x == 0) { a.work->psum[blockIdx.x] = s; a.work->pext[blockIdx.x] = col; }
  } else {
    block_fold<Add, Max>(s, mx);
    block_fold<Add>(cnt);
    if (threadIdx.x == 0) { a.work->psum[blockIdx.x] = s; a.work->pext[blockIdx.x] = mx; a.work->pcnt[blockIdx.x] = cnt; }
  }
}

template <bool SECOND>
__global__ __launch_bounds__(kBlock) void cas_finish_totals(CasWork* w, const int nb) {
  double s = thread_partials<Add>(w->psum, nb);
  if (SECOND) {
    double col = thread_partials<Min>(w->pext, nb);
    block_fold<Add, Min>(s, col);
    if (threadIdx.x == 0) { w->tot.ss = s; w->tot.col = col; }
    return;
  }
  double mx = thread_partials<Max>(w->pext, nb);
  u64 cnt = thread_partials<Add>(w->pcnt, nb);
  block_fold<Add, Max>(s, mx);
  block_fold<Add>(cnt);
  if (threadIdx.x == 0) {
    w->tot.m_c = cnt; w->tot.sum = s; w->tot.max = mx;
    w->tot.mean = s / (double)cnt;   // NaN without a counted column
  }
}

// ---- rows: workgroup r walks the columns of row r = (k, f).  The hit counts of a kTileEdge x kTileEdge window of the raster,
// anchored on the first impact the workgroup sees, are kept in LDS and flushed once (count * W); what falls outside the
// window goes to the map directly.  Integer adds: the map does not depend on the window or on the order.  (Against adds
// straight to the map the window measured the same on spread clouds and 22 times faster with every job in one cell:
// DESIGN.md 8.19.)
__global__ __launch_bounds__(kBlock) void cas_rows(const CasArgs a) {
  __shared__ unsigned int s_tile[kTileEdge * kTileEdge];
  __shared__ int s_origin;
  __shared__ unsigned int s_wcnt[kWaves];
  const int r = blockIdx.x, f = r % a.n_fragments, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t m = a.m, ld = a.ld, R = (int64_t)a.n_nodes * a.n_fragments;
  const ErplEdges ex = erpl_edges_of(a.g.lo_x, a.g.hi_x, a.g.bins_x), ey = erpl_edges_of(a.g.lo_y, a.g.hi_y, a.g.bins_y);
  const double* __restrict__ X = a.values + ((int64_t)ERPL_IIP_CH_X * R + r) * ld;
  const double* __restrict__ Y = a.values + ((int64_t)ERPL_IIP_CH_Y * R + r) * ld;
  const double* __restrict__ V = a.values + ((int64_t)ERPL_IIP_CH_VIMPACT * R + r) * ld;
  const double c_f = a.c_f[f], half_mass = a.half_mass[f];
  const u64 W = (u64)a.work->W[r];
  const int bins_y = a.g.bins_y;
  const int tile_x = a.g.bins_x < kTileEdge ? a.g.bins_x : kTileEdge, tile_y = bins_y < kTileEdge ? bins_y : kTileEdge;
  double2* __restrict__ dense = a.smooth ? a.pts + (int64_t)r * m : nullptr;
  for (int t = threadIdx.x; t < kTileEdge * kTileEdge; t += kBlock) s_tile[t] = 0u;
  if (threadIdx.x == 0) s_origin = -1;
  __syncthreads();
  u64 cnt[4] = {0ull, 0ull, 0ull, 0ull};
  double S = 0.0;
  int64_t running = 0;   // members of the group before this chunk
  for (int64_t base = 0; base < m; base += kBlock) {
    const int64_t j = base + threadIdx.x;
    const bool counted = j < m && (!a.mask || a.mask[j] == 0);
    const double x = counted ? X[j] : 0.0, y = counted ? Y[j] : 0.0, v = counted ? V[j] : 0.0;
    const int cls = counted ? erpl_cas_class(x, y, v, half_mass, a.ke_min) : 0;
    const bool landed = (cls & ERPL_CAS_LANDED) != 0, lethal = (cls & ERPL_CAS_LETHAL) != 0;
    int32_t cell = 0;
    const bool inside = lethal && erpl_cas_cell(a.g, ex, ey, x, y, &cell);
    S += inside ? c_f * a.population[cell] : 0.0;
    const u64 lm = __ballot(lethal), im = __ballot(inside);
    cnt[0] += (u64)__popcll(__ballot(landed));
    cnt[1] += (u64)__popcll(lm);
    cnt[2] += (u64)__popcll(lm & ~im);
    cnt[3] += (u64)__popcll(__ballot(counted && !landed));
    if (W != 0ull && im != 0ull) {
      const int cx = cell / bins_y, cy = cell % bins_y;
      const int lead = __ffsll((long long)im) - 1;
      int org = 0;
      if (lane == lead) {
        org = __hip_atomic_load(&s_origin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (org < 0) {
          int ox = cx - tile_x / 2, oy = cy - tile_y / 2;
          ox = ox < 0 ? 0 : (ox > a.g.bins_x - tile_x ? a.g.bins_x - tile_x : ox);
          oy = oy < 0 ? 0 : (oy > bins_y - tile_y ? bins_y - tile_y : oy);
          const int mine = ox * 65536 + oy;
          const int old = atomicCAS(&s_origin, -1, mine);
          org = old < 0 ? mine : old;
        }
      }
      org = __shfl(org, lead);
      const int lx = cx - org / 65536, ly = cy - org % 65536;
      if (inside) {
        if (lx >= 0 && lx < tile_x && ly >= 0 && ly < tile_y) atomicAdd(&s_tile[lx * tile_y + ly], 1u);
        else atomicAdd(&a.words[cell], W);
      }
    }
    if (a.smooth) {   // stable: the members of the waves before, then the lanes before
      if (lane == 0) s_wcnt[wave] = (unsigned int)__popcll(lm);
      __syncthreads();
      int64_t before = running, all = 0;
      for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += s_wcnt[w];
        all += s_wcnt[w];
      }
      if (lethal) dense[before + __popcll(lm & ((1ull << lane) - 1ull))] = make_double2(x, y);   // below cnt[1] <= m
      running += all;
      __syncthreads();   // s_wcnt is written again in the next chunk
    }
  }
  block_fold<Add>(S);
  const u64 c = counters_fold(cnt);   // its barrier also orders the tile's adds before the flush
  CasRow& rec = a.work->row[r];
  if (threadIdx.x < 4) rec.cnt[threadIdx.x] = c;
  if (threadIdx.x == 0) rec.S = S;
  const int org = s_origin;
  if (org >= 0)
    for (int t = threadIdx.x; t < tile_x * tile_y; t += kBlock) {
      const unsigned int hits = s_tile[t];
      if (hits) atomicAdd(&a.words[(org / 65536 + t / tile_y) * bins_y + org % 65536 + t % tile_y], (u64)hits * W);
    }
}

// ---- groups: workgroup r, over the dense members of row r
__global__ __launch_bounds__(kBlock) void cas_groups(const CasArgs a) {
  __shared__ double s_map[5];   // mean_x, mean_y, w11, w21, w22
  __shared__ int s_solid;
  const int r = blockIdx.x;
  CasRow& rec = a.work->row[r];
  const int64_t n = (int64_t)rec.cnt[1];
  double2* __restrict__ p = a.pts + (int64_t)r * a.m;
  double sx = 0.0, sy = 0.0;
  for (int64_t d = threadIdx.x; d < n; d += kBlock) { sx += p[d].x; sy += p[d].y; }
  block_fold<Add, Add>(sx, sy);
  if (threadIdx.x == 0) { s_map[0] = sx / (double)n; s_map[1] = sy / (double)n; }   // NaN for an empty group
  __syncthreads();
  const double mx = s_map[0], my = s_map[1];
  double sxx = 0.0, sxy = 0.0, syy = 0.0;
  for (int64_t d = threadIdx.x; d < n; d += kBlock) {
    const double dx = p[d].x - mx, dy = p[d].y - my;
    sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
  }
  block_fold<Add, Add, Add>(sxx, sxy, syy);
  if (threadIdx.x == 0) {
    const double nan = NAN;
    bool solid = false;
    rec.mean_x = mx; rec.mean_y = my;
    rec.hxx = rec.hxy = rec.hyy = nan;
    rec.w11 = rec.w21 = rec.w22 = 0.0; rec.norm = 0.0;
    if (n > 0) {
      const double dof = (double)(n - 1);
      const double cxx = n < 2 ? 0.0 : sxx / dof, cxy = n < 2 ? 0.0 : sxy / dof, cyy = n < 2 ? 0.0 : syy / dof;
      const double factor = a.bw_scale * pow((double)n, -1.0 / 6.0), f2 = factor * factor, floor2 = a.h_floor * a.h_floor;
      const double hxx = f2 * cxx + floor2, hxy = f2 * cxy, hyy = f2 * cyy + floor2;
      rec.hxx = hxx; rec.hxy = hxy; rec.hyy = hyy;
      const double det = hxx * hyy - hxy * hxy;
      // H = C C': u = dx / c11, v = (dy - c21 u) / c22
      const double c11 = sqrt(hxx), c21 = hxy / c11, c22 = sqrt(hyy - c21 * c21);
      solid = finite_bits(hxx) && finite_bits(hxy) && finite_bits(hyy) && finite_bits(det) && hxx > 0.0 && det > 0.0 &&
              finite_bits(c22) && c22 > 0.0;
      if (solid) {
        rec.w11 = 1.0 / c11; rec.w22 = 1.0 / c22; rec.w21 = -c21 * rec.w11 * rec.w22;
        rec.norm = (a.work->w[r] / (double)a.work->tot.m_c) / ((2.0 * M_PI) * sqrt(det));
      }
    }
    rec.n_use = solid ? (u64)n : 0ull;
    s_map[2] = rec.w11; s_map[3] = rec.w21; s_map[4] = rec.w22;
    s_solid = solid ? 1 : 0;
  }
  __syncthreads();
  if (!s_solid) return;
  const double w11 = s_map[2], w21 = s_map[3], w22 = s_map[4];
  for (int64_t d = threadIdx.x; d < n; d += kBlock) {
    const double dx = p[d].x - mx, dy = p[d].y - my;
    p[d] = make_double2(w11 * dx, __builtin_fma(w21, dx, w22 * dy));
  }
}

// ---- pairs: workgroup (bx, by) adds the groups of the rows by * per_slice .. min(R, (by + 1) * per_slice) - 1, in row order
// and each in member order, for the cells bx * ERPL_CAS_TILE + k * kBlock + thread, k < ERPL_DENS_Q, into partial[by][cell].
static_assert(ERPL_CAS_TILE == ERPL_DENS_Q * kBlock, "a thread owns ERPL_DENS_Q cells of the workgroup's tile");
__global__ __launch_bounds__(kBlock) void cas_pairs(const CasArgs a, const int per_slice, double* __restrict__ partial) {
  __shared__ double2 s_src[ERPL_CAS_TILE];
  const int tid = threadIdx.x, bins_y = a.g.bins_y;
  const int64_t cells = (int64_t)a.g.bins_x * bins_y, m = a.m;
  const int R = a.n_nodes * a.n_fragments;
  const int first = (int)blockIdx.y * per_slice, last = first + per_slice < R ? first + per_slice : R;
  const ErplEdges ex = erpl_edges_of(a.g.lo_x, a.g.hi_x, a.g.bins_x), ey = erpl_edges_of(a.g.lo_y, a.g.hi_y, bins_y);
  const int64_t q0 = (int64_t)blockIdx.x * ERPL_CAS_TILE + tid;
  double gx[ERPL_DENS_Q], gy[ERPL_DENS_Q], tot[ERPL_DENS_Q];
#pragma unroll
  for (int k = 0; k < ERPL_DENS_Q; ++k) {
    const int64_t q = q0 + (int64_t)k * kBlock;
    const bool have = q < cells;   // a lane without a cell computes and stores nothing
    gx[k] = have ? erpl_cas_centre(ex, (int)(q / bins_y)) : 0.0;
    gy[k] = have ? erpl_cas_centre(ey, (int)(q % bins_y)) : 0.0;
    tot[k] = 0.0;
  }
  for (int r = first; r < last; ++r) {
    const CasRow& rec = a.work->row[r];
    const int64_t n = (int64_t)rec.n_use;   // uniform over the workgroup: so are the barriers below
    if (n == 0) continue;
    const double mx = rec.mean_x, my = rec.mean_y, w11 = rec.w11, w21 = rec.w21, w22 = rec.w22;
    const double2* __restrict__ src = a.pts + (int64_t)r * m;
    double qu[ERPL_DENS_Q], qv[ERPL_DENS_Q], acc[ERPL_DENS_Q];
#pragma unroll
    for (int k = 0; k < ERPL_DENS_Q; ++k) {
      const double dx = gx[k] - mx, dy = gy[k] - my;
      qu[k] = w11 * dx; qv[k] = __builtin_fma(w21, dx, w22 * dy); acc[k] = 0.0;
    }
    for (int64_t base = 0; base < n; base += ERPL_CAS_TILE) {
      const int cnt = (int)(n - base < ERPL_CAS_TILE ? n - base : ERPL_CAS_TILE);
      __syncthreads();   // the tile before has been read
      for (int j = tid; j < cnt; j += kBlock) s_src[j] = src[base + j];
      __syncthreads();
      for (int j = 0; j < cnt; ++j) {
        const double2 s = s_src[j];   // one address per wave: a broadcast
#pragma unroll
        for (int k = 0; k < ERPL_DENS_Q; ++k) {
          const double du = qu[k] - s.x, dv = qv[k] - s.y;
          const double e = __builtin_fma(dv, dv, du * du);
          acc[k] += exp(-0.5 * e);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < ERPL_DENS_Q; ++k) tot[k] += rec.norm * acc[k];
  }
#pragma unroll
  for (int k = 0; k < ERPL_DENS_Q; ++k) {
    const int64_t q = q0 + (int64_t)k * kBlock;
    if (q < cells) partial[(int64_t)blockIdx.y * cells + q] = tot[k];
  }
}

__global__ __launch_bounds__(kBlock) void cas_fold(const double* __restrict__ partial, const int slices, const int64_t cells,
                                                   double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < cells; q += stride) {
    double s = partial[q];
    for (int k = 1; k < slices; ++k) s += partial[(int64_t)k * cells + q];
    out[q] = s;
  }
}

// ---------------------------------------------------------------- the refusals, in the order of the header

int check_amount(double v, const char* name, int f) {
  if (std::isfinite(v) && v >= 0.0) return ERPL_OK;
  return erpl_fail(ERPL_ERR_INVALID, "spec->%s[%d] = %g: finite and >= 0", name, f, v);
}

int casualty_check(const double* values, const erpl_casualty_spec* s, const double* p_fail, const double* population,
                   const erpl_casualty* result, int64_t ld, int64_t m) {
  if (!values) return erpl_fail(ERPL_ERR_INVALID, "values is NULL");
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (!p_fail) return erpl_fail(ERPL_ERR_INVALID, "p_fail is NULL");
  if (!population) return erpl_fail(ERPL_ERR_INVALID, "population is NULL");
  if (!result) return erpl_fail(ERPL_ERR_INVALID, "result is NULL");
  if (s->n_nodes < 1 || s->n_nodes > ERPL_IIP_MAX_NODES)
    return erpl_fail(ERPL_ERR_INVALID, "spec->n_nodes = %d out of range 1..%d", s->n_nodes, ERPL_IIP_MAX_NODES);
  if (s->n_fragments < 1 || s->n_fragments > ERPL_DEBRIS_MAX_FRAGMENTS)
    return erpl_fail(ERPL_ERR_INVALID, "spec->n_fragments = %d out of range 1..%d", s->n_fragments, ERPL_DEBRIS_MAX_FRAGMENTS);
  if ((int64_t)s->n_nodes * s->n_fragments > ERPL_CORRIDOR_MAX_NODES)
    return erpl_fail(ERPL_ERR_INVALID, "n_nodes * n_fragments = %lld: the product is at most %d rows per channel",
                     (long long)s->n_nodes * s->n_fragments, ERPL_CORRIDOR_MAX_NODES);
  for (int f = 0; f < s->n_fragments; ++f) {
    ERPL_TRY(check_amount(s->pieces[f], "pieces", f));
    ERPL_TRY(check_amount(s->area[f], "area", f));
    ERPL_TRY(check_amount(s->mass[f], "mass", f));
  }
  if (!(std::isfinite(s->ke_min) && s->ke_min >= 0.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->ke_min = %g: finite and >= 0", s->ke_min);
  if (s->bins_x < 1 || s->bins_x > ERPL_CASUALTY_MAX_GRID)
    return erpl_fail(ERPL_ERR_INVALID, "spec->bins_x = %d out of range 1..%d", s->bins_x, ERPL_CASUALTY_MAX_GRID);
  if (s->bins_y < 1 || s->bins_y > ERPL_CASUALTY_MAX_GRID)
    return erpl_fail(ERPL_ERR_INVALID, "spec->bins_y = %d out of range 1..%d", s->bins_y, ERPL_CASUALTY_MAX_GRID);
  if (!(std::isfinite(s->lo_x) && std::isfinite(s->hi_x) && s->lo_x < s->hi_x && std::isfinite(s->hi_x - s->lo_x)))
    return erpl_fail(ERPL_ERR_INVALID, "spec->lo_x = %g, spec->hi_x = %g: finite and lo_x < hi_x", s->lo_x, s->hi_x);
  if (!(std::isfinite(s->lo_y) && std::isfinite(s->hi_y) && s->lo_y < s->hi_y && std::isfinite(s->hi_y - s->lo_y)))
    return erpl_fail(ERPL_ERR_INVALID, "spec->lo_y = %g, spec->hi_y = %g: finite and lo_y < hi_y", s->lo_y, s->hi_y);
  if (s->smooth != 0 && s->smooth != 1) return erpl_fail(ERPL_ERR_INVALID, "spec->smooth = %d: 0 or 1", s->smooth);
  if (!(std::isfinite(s->bw_scale) && s->bw_scale > 0.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->bw_scale = %g: finite and > 0", s->bw_scale);
  if (!(std::isfinite(s->h_floor) && s->h_floor > 0.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->h_floor = %g: finite and > 0", s->h_floor);
  if (s->n_levels < 0 || s->n_levels > ERPL_CASUALTY_MAX_LEVELS)
    return erpl_fail(ERPL_ERR_INVALID, "spec->n_levels = %d outside 0..%d", s->n_levels, ERPL_CASUALTY_MAX_LEVELS);
  for (int k = 0; k < s->n_levels; ++k)
    if (!(s->level[k] > 0.0 && s->level[k] < 1.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->level[%d] = %g outside (0, 1)", k, s->level[k]);
  double sum = 0.0;
  for (int k = 0; k < s->n_nodes; ++k) {
    if (!(std::isfinite(p_fail[k]) && p_fail[k] >= 0.0)) return erpl_fail(ERPL_ERR_INVALID, "p_fail[%d] = %g: finite and >= 0", k, p_fail[k]);
    sum += p_fail[k];
  }
  if (!(sum <= 1.0 + 1e-12)) return erpl_fail(ERPL_ERR_INVALID, "p_fail sums to %.17g: the probabilities of break-up are at most 1 together", sum);
  if (m <= 0 || m > 2147483647LL) return erpl_fail(ERPL_ERR_INVALID, "m = %lld outside 1..2^31 - 1", (long long)m);
  if (ld < m) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below m = %lld", (long long)ld, (long long)m);
  const int q = erpl_cas_q(m, s->n_nodes, s->n_fragments);
  if (q < ERPL_CAS_Q_LEAST)
    return erpl_fail(ERPL_ERR_INVALID, "Q = %d: m * n_nodes * n_fragments leaves fewer than %d bits for the weights of the map", q, ERPL_CAS_Q_LEAST);
  return ERPL_OK;
}

size_t round_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int erpl_mc_casualty_defaults(erpl_casualty_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  memset(spec, 0, sizeof(*spec));
  spec->n_nodes = 16; spec->n_fragments = 1;
  spec->pieces[0] = 1.0; spec->area[0] = 1.0; spec->mass[0] = 1.0;
  spec->ke_min = 15.0;
  spec->bins_x = spec->bins_y = 64;
  spec->lo_x = spec->lo_y = -1000.0; spec->hi_x = spec->hi_y = 1000.0;
  spec->smooth = 1; spec->bw_scale = 1.0; spec->h_floor = 1.0;
  spec->n_levels = 2;
  spec->level[0] = 1e-6; spec->level[1] = 1e-5;
  return ERPL_OK;
}

int erpl_mc_casualty(erpl_ctx* c, const double* values, int64_t ld, int64_t m, const uint8_t* mask, const erpl_casualty_spec* spec,
                     const double* p_fail, const double* population, double* ec_traj, double* per_node, double* per_fragment,
                     double* groups, double* hazard, int64_t* hazard_words, double* risk_smooth, erpl_casualty* result,
                     void* stream) {
  ERPL_TRY(casualty_check(values, spec, p_fail, population, result, ld, m));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int K = spec->n_nodes, F = spec->n_fragments, R = K * F;
  const int64_t cells = (int64_t)spec->bins_x * spec->bins_y;
  const bool smooth = spec->smooth != 0;
  int per_slice = 0;
  const int slices = erpl_cas_slices(R, cells, &per_slice);

  // the buffer: [work][words cells][e_j m unless the caller keeps them][members R * m][partial slices * cells][risk cells]
  size_t need = round_up(sizeof(CasWork));
  const size_t at_words = need; need += round_up((size_t)cells * 8);
  const size_t at_ec = need; if (!ec_traj) need += round_up((size_t)m * 8);
  const size_t at_pts = need; if (smooth) need += round_up((size_t)R * (size_t)m * 16);
  const size_t at_part = need; if (smooth) need += round_up((size_t)slices * (size_t)cells * 8);
  const size_t at_risk = need; if (smooth) need += round_up((size_t)cells * 8);
  ERPL_TRY(c->casualty.grow(need));
  char* buf = c->casualty.buf;

  CasArgs a;
  memset(&a, 0, sizeof(a));
  a.values = values; a.mask = mask; a.population = population; a.work = (CasWork*)buf;
  a.words = (unsigned long long*)(buf + at_words);
  a.ec = ec_traj ? ec_traj : (double*)(buf + at_ec);
  a.pts = smooth ? (double2*)(buf + at_pts) : nullptr;
  a.m = m; a.ld = ld; a.n_nodes = K; a.n_fragments = F; a.smooth = smooth ? 1 : 0;
  a.ke_min = spec->ke_min; a.bw_scale = spec->bw_scale; a.h_floor = spec->h_floor;
  a.g.lo_x = spec->lo_x; a.g.hi_x = spec->hi_x; a.g.lo_y = spec->lo_y; a.g.hi_y = spec->hi_y;
  a.g.bins_x = spec->bins_x; a.g.bins_y = spec->bins_y;
  for (int f = 0; f < F; ++f) { a.c_f[f] = spec->pieces[f] * spec->area[f]; a.half_mass[f] = 0.5 * spec->mass[f]; }
  double* partial = (double*)(buf + at_part);
  double* risk = (double*)(buf + at_risk);

  // what the host settles first: w_kf, w_max, Q and the integer weights
  std::vector<double> w((size_t)R);
  std::vector<long long> W((size_t)R);
  double w_max = 0.0;
  for (int k = 0; k < K; ++k)
    for (int f = 0; f < F; ++f) {
      const double v = p_fail[k] * a.c_f[f];
      w[(size_t)k * F + f] = v;
      w_max = v > w_max ? v : w_max;
    }
  const int Q = erpl_cas_q(m, K, F);
  for (int r = 0; r < R; ++r) W[(size_t)r] = (long long)erpl_cas_weight(w[(size_t)r], w_max, Q);

  std::vector<double> pop((size_t)cells);
  unsigned int bad = 0u;
  HIP_TRY(hipMemsetAsync(a.work, 0, offsetof(CasWork, psum), st));
  HIP_TRY(hipMemcpyAsync(a.work->p_fail, p_fail, (size_t)K * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(a.work->w, w.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(a.work->W, W.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(cas_population, dim3(grid_of(cells)), dim3(kBlock), 0, st, population, cells, a.work);
  KERNEL_TRY((int)hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&bad, &a.work->bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(pop.data(), population, (size_t)cells * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad) return erpl_fail(ERPL_ERR_INVALID, "population: %u of %lld entries are negative or not finite", bad, (long long)cells);

  const int nb = grid_of(m);
  HIP_TRY(hipMemsetAsync(a.words, 0, (size_t)cells * 8, st));
  hipLaunchKernelGGL(cas_traj, dim3(nb), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(cas_totals<false>, dim3(nb), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(cas_finish_totals<false>, dim3(1), dim3(kBlock), 0, st, a.work, nb);
  hipLaunchKernelGGL(cas_totals<true>, dim3(nb), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(cas_finish_totals<true>, dim3(1), dim3(kBlock), 0, st, a.work, nb);
  hipLaunchKernelGGL(cas_rows, dim3(R), dim3(kBlock), 0, st, a);
  if (smooth) {
    hipLaunchKernelGGL(cas_groups, dim3(R), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(cas_pairs, dim3((unsigned)((cells + ERPL_CAS_TILE - 1) / ERPL_CAS_TILE), (unsigned)slices), dim3(kBlock), 0, st,
                       a, per_slice, partial);
    hipLaunchKernelGGL(cas_fold, dim3(grid_of(cells)), dim3(kBlock), 0, st, partial, slices, cells, risk);
  }
  KERNEL_TRY((int)hipGetLastError());

  std::vector<CasRow> rows((size_t)R);
  std::vector<long long> words((size_t)cells);
  std::vector<double> rs(smooth ? (size_t)cells : 0);
  CasTotals tot;
  HIP_TRY(hipMemcpyAsync(&tot, &a.work->tot, sizeof(tot), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(rows.data(), a.work->row, (size_t)R * sizeof(CasRow), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(words.data(), a.words, (size_t)cells * 8, hipMemcpyDeviceToHost, st));
  if (smooth) HIP_TRY(hipMemcpyAsync(rs.data(), risk, (size_t)cells * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  // what the host finishes in double, in index order
  const double nan = NAN;
  const int64_t m_c = (int64_t)tot.m_c;
  const double mc = (double)m_c;
  memset(result, 0, sizeof(*result));
  result->m_c = m_c; result->q = Q; result->w_max = w_max;
  result->ec = m_c > 0 ? tot.mean : nan;
  result->ec_std = m_c > 0 ? sqrt(tot.ss / (double)(m_c - 1)) : nan;
  result->ec_se = m_c > 0 ? result->ec_std / sqrt(mc) : nan;
  result->ec_max = m_c > 0 ? tot.max : nan;
  result->ec_max_col = m_c > 0 ? (int64_t)tot.col : -1;
  for (int r = 0; r < R; ++r) {
    result->landed += (int64_t)rows[(size_t)r].cnt[0]; result->lethal += (int64_t)rows[(size_t)r].cnt[1];
    result->off_grid += (int64_t)rows[(size_t)r].cnt[2]; result->missing += (int64_t)rows[(size_t)r].cnt[3];
  }
  if (per_node)
    for (int k = 0; k < K; ++k) {
      double s = 0.0, cnt[4] = {0.0, 0.0, 0.0, 0.0};
      for (int f = 0; f < F; ++f) {
        const CasRow& rec = rows[(size_t)k * F + f];
        s += rec.S;
        for (int t = 0; t < 4; ++t) cnt[t] += (double)rec.cnt[t];
      }
      per_node[k] = s / mc;
      for (int t = 0; t < 4; ++t) per_node[(size_t)(t + 1) * K + k] = cnt[t];
    }
  if (per_fragment)
    for (int f = 0; f < F; ++f) {
      double s = 0.0, cnt[4] = {0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < K; ++k) {
        const CasRow& rec = rows[(size_t)k * F + f];
        s += p_fail[k] * rec.S;
        for (int t = 0; t < 4; ++t) cnt[t] += (double)rec.cnt[t];
      }
      per_fragment[f] = s / mc;
      for (int t = 0; t < 4; ++t) per_fragment[(size_t)(t + 1) * F + f] = cnt[t];
    }
  double denom = 0.0;
  for (int r = 0; r < R; ++r) {
    const CasRow& rec = rows[(size_t)r];
    denom += (w[(size_t)r] * (double)rec.cnt[1]) / mc;
    if (!groups) continue;
    double* g = groups + (size_t)r * ERPL_CASUALTY_GROUP_DIM;
    const bool have = smooth && rec.cnt[1] > 0;
    g[ERPL_CASUALTY_G_COUNT] = (double)rec.cnt[1]; g[ERPL_CASUALTY_G_S] = rec.S;
    g[ERPL_CASUALTY_G_MEAN_X] = have ? rec.mean_x : nan; g[ERPL_CASUALTY_G_MEAN_Y] = have ? rec.mean_y : nan;
    g[ERPL_CASUALTY_G_HXX] = have ? rec.hxx : nan; g[ERPL_CASUALTY_G_HXY] = have ? rec.hxy : nan;
    g[ERPL_CASUALTY_G_HYY] = have ? rec.hyy : nan; g[ERPL_CASUALTY_G_W] = w[(size_t)r];
  }
  const double area = erpl_cas_cell_area(a.g), scale = erpl_cas_scale(w_max, Q, m_c);
  result->cell_area = area;
  double ec_map = 0.0, ec_smooth = 0.0, mass = 0.0;
  int64_t over[ERPL_CASUALTY_MAX_LEVELS] = {0}, over_s[ERPL_CASUALTY_MAX_LEVELS] = {0};
  for (int64_t q = 0; q < cells; ++q) {
    const double hz = (double)words[(size_t)q] * scale, risk_c = hz / area;
    if (hazard) hazard[q] = hz;
    if (hazard_words) hazard_words[q] = (int64_t)words[(size_t)q];
    ec_map += hz * pop[(size_t)q];
    for (int i = 0; i < spec->n_levels; ++i) over[i] += risk_c >= spec->level[i] ? 1 : 0;
    if (!smooth) continue;
    const double v = rs[(size_t)q];
    if (risk_smooth) risk_smooth[q] = v;
    ec_smooth += (v * pop[(size_t)q]) * area;
    mass += v * area;
    for (int i = 0; i < spec->n_levels; ++i) over_s[i] += v >= spec->level[i] ? 1 : 0;
  }
  result->ec_map = ec_map;
  result->ec_smooth = smooth ? ec_smooth : nan;
  result->mix_mass = smooth && denom > 0.0 ? mass / denom : nan;
  for (int i = 0; i < ERPL_CASUALTY_MAX_LEVELS; ++i) {
    result->level_area[i] = i < spec->n_levels ? (double)over[i] * area : 0.0;
    result->level_area_smooth[i] = i < spec->n_levels ? (smooth ? (double)over_s[i] * area : nan) : 0.0;
  }
  return ERPL_OK;
}

}  // extern "C"
