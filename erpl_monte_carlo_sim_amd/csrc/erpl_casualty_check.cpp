// erpl_casualty_check — erpl_casualty.h on the host alone (no HIP, no library): what must hold before a kernel runs anywhere.
//   1. Q and the integer weights: Q = 40 for small shapes, falls with bit_length(m * nodes * fragments), is 19 at the largest
//      shape the call admits (so the refusal below 16 cannot be reached through it) and below 16 beyond; W = 2^Q for w = w_max,
//      0 for w = 0 and for w_max = 0, monotone in w; all jobs at 2^Q in one cell stay below 2^62
//   2. the lethal rule at, one double below and one double above ke_min; ke_min = 0 makes every landed job lethal; a NaN or an
//      infinity in any of the three values is not landed
//   3. the cell of a point on every edge of a raster - the last edge included - and just off both ends
//   4. the centres: inside their cell, cell i's own bin, symmetric about the middle of the range
//   5. a permuted job order gives the same map bytes; the hazard of a job is c_f * population[cell]
//   6. the slices of the smoothing pass cover every row once
// Prints one ok line per part; exit status 1 on the first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_casualty.h"

namespace {
#define REQUIRE(cond, ...)                     \
  do {                                         \
    if (!(cond)) {                             \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
      return false;                            \
    }                                          \
  } while (0)

bool check_weights() {
  REQUIRE(erpl_cas_q(1, 1, 1) == 40 && erpl_cas_q(8192, 16, 8) == 40, "Q of small shapes");
  REQUIRE(erpl_cas_q((1ll << 22) - 1, 1, 1) == 40 && erpl_cas_q(1ll << 22, 1, 1) == 39, "Q about 2^22 jobs");
  REQUIRE(erpl_cas_q((1ll << 31) - 1, ERPL_IIP_MAX_NODES, 1) == 19, "Q at the largest shape: %d",
          erpl_cas_q((1ll << 31) - 1, ERPL_IIP_MAX_NODES, 1));
  REQUIRE(erpl_cas_q((1ll << 31) - 1, 64, ERPL_DEBRIS_MAX_FRAGMENTS) == 19, "Q at 64 x 64 rows");
  REQUIRE(erpl_cas_q(1ll << 46, 1, 1) == 15 && erpl_cas_q(1ll << 46, 1, 1) < ERPL_CAS_Q_LEAST, "Q beyond the admitted shapes");
  for (int q = 15; q <= 40; ++q) {
    REQUIRE(erpl_cas_weight(3.5, 3.5, q) == (1ll << q), "W of w_max at Q = %d", q);
    REQUIRE(erpl_cas_weight(0.0, 3.5, q) == 0 && erpl_cas_weight(1.0, 0.0, q) == 0, "W of zero at Q = %d", q);
    int64_t before = 0;
    for (int i = 0; i <= 1000; ++i) {
      const int64_t w = erpl_cas_weight(1e-3 * i * 0.7, 0.7, q);
      REQUIRE(w >= before && w <= (1ll << q), "W is not monotone at %d, Q = %d", i, q);
      before = w;
    }
  }
  REQUIRE(erpl_cas_weight(0.25, 1.0, 40) == (1ll << 38) && erpl_cas_weight(1.0, 3.0, 16) == 21845, "W of a quarter and of a third");
  // every job of the largest shape at the largest weight in one cell
  const int q = erpl_cas_q((1ll << 31) - 1, ERPL_IIP_MAX_NODES, 1);
  const long double most = (long double)((1ll << 31) - 1) * ERPL_IIP_MAX_NODES * (long double)(1ll << q);
  REQUIRE(most < 0x1p62L, "the map can overflow");
  REQUIRE(erpl_cas_scale(2.0, 3, 4) == 0.0625 && erpl_cas_scale(2.0, 3, 0) == 0.0, "the scale of the map");
  printf("ok weights\n");
  return true;
}

bool check_lethal() {
  const double mass = 0.37, ke = 15.0, half = 0.5 * mass;
  // the smallest v with half * (v * v) >= ke, by bisection on the doubles
  double lo = 0.0, hi = 100.0;
  while (nextafter(lo, hi) < hi) {
    const double mid = lo + 0.5 * (hi - lo);
    if (half * (mid * mid) >= ke) hi = mid; else lo = mid;
  }
  const int both = ERPL_CAS_LANDED | ERPL_CAS_LETHAL;
  REQUIRE(erpl_cas_class(1.0, 2.0, hi, half, ke) == both, "at the threshold");
  REQUIRE(erpl_cas_class(1.0, 2.0, lo, half, ke) == ERPL_CAS_LANDED, "one double below the threshold");
  REQUIRE(erpl_cas_class(1.0, 2.0, nextafter(hi, 1e9), half, ke) == both, "one double above the threshold");
  REQUIRE(erpl_cas_class(1.0, 2.0, 0.0, half, 0.0) == both && erpl_cas_class(1.0, 2.0, 0.0, 0.0, 0.0) == both, "ke_min = 0");
  REQUIRE(erpl_cas_class(1.0, 2.0, 0.0, half, 5e-324) == ERPL_CAS_LANDED, "a job at rest under a positive ke_min");
  const double bad[3] = {NAN, INFINITY, -INFINITY};
  for (double b : bad) {
    REQUIRE(erpl_cas_class(b, 2.0, 3.0, half, 0.0) == 0 && erpl_cas_class(1.0, b, 3.0, half, 0.0) == 0 &&
            erpl_cas_class(1.0, 2.0, b, half, 0.0) == 0, "a job that is not finite");
  }
  printf("ok lethal\n");
  return true;
}

bool check_cells() {
  const ErplCasRaster rasters[4] = {{-3.0, 7.0, 0.1, 0.7, 7, 3}, {0.0, 1.0, -1.0, 1.0, 1, 1}, {-1e3, 1e3, -2e3, 5e2, 64, 48},
                                    {0.3, 0.3 + 1024 * 0.1, -7.7, 9.1, 1024, 5}};
  for (const ErplCasRaster& g : rasters) {
    const ErplEdges ex = erpl_edges_of(g.lo_x, g.hi_x, g.bins_x), ey = erpl_edges_of(g.lo_y, g.hi_y, g.bins_y);
    REQUIRE(ex[0] == g.lo_x && ex[g.bins_x] == g.hi_x && ey[0] == g.lo_y && ey[g.bins_y] == g.hi_y, "the outer edges");
    int32_t cell = -1;
    for (int i = 0; i <= g.bins_x; ++i)
      for (int j = 0; j <= g.bins_y; ++j) {
        REQUIRE(erpl_cas_cell(g, ex, ey, ex[i], ey[j], &cell), "an edge point is off the raster");
        const int wx = i < g.bins_x ? i : g.bins_x - 1, wy = j < g.bins_y ? j : g.bins_y - 1;   // the last edge closes the last cell
        REQUIRE(cell == wx * g.bins_y + wy, "edge (%d, %d) in cell %d, not %d", i, j, cell, wx * g.bins_y + wy);
      }
    cell = -1;
    REQUIRE(!erpl_cas_cell(g, ex, ey, nextafter(g.lo_x, -INFINITY), ey[0], &cell) && !erpl_cas_cell(g, ex, ey, nextafter(g.hi_x, INFINITY), ey[0], &cell) &&
            !erpl_cas_cell(g, ex, ey, ex[0], nextafter(g.lo_y, -INFINITY), &cell) && !erpl_cas_cell(g, ex, ey, ex[0], nextafter(g.hi_y, INFINITY), &cell) &&
            cell == -1, "a point just off the raster");
    // the centres
    for (int i = 0; i < g.bins_x; ++i) {
      const double cx = erpl_cas_centre(ex, i);
      REQUIRE(cx > ex[i] && cx < ex[i + 1], "centre %d of x outside its cell", i);
      REQUIRE(erpl_cas_cell(g, ex, ey, cx, erpl_cas_centre(ey, 0), &cell) && cell == i * g.bins_y, "centre %d of x in cell %d", i, cell);
      const double mirror = erpl_cas_centre(ex, g.bins_x - 1 - i), mid = 0.5 * (g.lo_x + g.hi_x);
      REQUIRE(fabs((cx - mid) + (mirror - mid)) <= 4e-16 * (fabs(g.lo_x) + fabs(g.hi_x)) * g.bins_x, "the centres of x are not symmetric at %d", i);
    }
    const double want = (g.hi_x - g.lo_x) * (g.hi_y - g.lo_y) / ((double)g.bins_x * g.bins_y);
    REQUIRE(fabs(erpl_cas_cell_area(g) - want) <= 4e-16 * want, "the cell area");
  }
  printf("ok cells and centres\n");
  return true;
}

bool check_map_order() {
  const ErplCasRaster g = {-10.0, 10.0, -5.0, 5.0, 9, 5};
  const int n = 4000, cells = g.bins_x * g.bins_y;
  std::vector<double> pop((size_t)cells);
  for (int c = 0; c < cells; ++c) pop[(size_t)c] = 1e-4 * (1 + c % 7);
  std::vector<double> x((size_t)n), y((size_t)n), v((size_t)n);
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto next = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) * 0x1p-53; };
  for (int i = 0; i < n; ++i) {
    x[(size_t)i] = i % 11 == 0 ? NAN : -12.0 + 24.0 * next();   // some off the raster, some missing
    y[(size_t)i] = -6.0 + 12.0 * next();
    v[(size_t)i] = 20.0 * next();
  }
  const int q = erpl_cas_q(n, 1, 1);
  const int64_t weight = erpl_cas_weight(0.3, 0.7, q);
  std::vector<int64_t> a((size_t)cells, 0), b((size_t)cells, 0);
  double ha = 0.0;
  int lethal = 0, cls = 0;
  for (int i = 0; i < n; ++i) {
    const double h = erpl_cas_job_host(g, x[(size_t)i], y[(size_t)i], v[(size_t)i], 0.5, 15.0, 2.5, weight, pop.data(), a.data(), &cls);
    REQUIRE(h >= 0.0 && (h == 0.0 || (cls & ERPL_CAS_LETHAL)), "a hazard without a lethal job");
    ha += h;
    lethal += (cls & ERPL_CAS_LETHAL) ? 1 : 0;
  }
  for (int i = 0; i < n; ++i) {   // another order: a stride coprime to n
    const size_t k = (size_t)(((int64_t)i * 1237 + 5) % n);
    erpl_cas_job_host(g, x[k], y[k], v[k], 0.5, 15.0, 2.5, weight, pop.data(), b.data(), nullptr);
  }
  REQUIRE(memcmp(a.data(), b.data(), (size_t)cells * sizeof(int64_t)) == 0, "the map depends on the order of the jobs");
  int64_t total = 0;
  double from_map = 0.0;
  for (int c = 0; c < cells; ++c) { total += a[(size_t)c]; from_map += (double)(a[(size_t)c] / weight) * (2.5 * pop[(size_t)c]); }
  REQUIRE(total % weight == 0 && total / weight > 0 && total / weight <= lethal, "the map holds %lld, not a multiple of the weight", (long long)total);
  REQUIRE(fabs(from_map - ha) <= 1e-12 * ha, "the hazards %.17g do not add up to the map's %.17g", ha, from_map);
  printf("ok map order (%d lethal jobs, %lld on the raster)\n", lethal, (long long)(total / weight));
  return true;
}

bool check_slices() {
  const int rows[6] = {1, 3, 15, 128, 4095, 4096};
  const int64_t cells[6] = {1, 15, 3072, 65536, 1 << 20, 1023};
  for (int R : rows)
    for (int64_t c : cells) {
      int per = 0;
      const int s = erpl_cas_slices(R, c, &per);
      REQUIRE(per >= 1 && s >= 1 && (int64_t)s * per >= R && (int64_t)(s - 1) * per < R, "rows %d, cells %lld: %d slices of %d", R, (long long)c, s, per);
      REQUIRE(s <= R && s <= ERPL_CAS_TARGET_BLOCKS, "rows %d, cells %lld: %d slices", R, (long long)c, s);
    }
  int per = 0;
  REQUIRE(erpl_cas_slices(128, 65536, &per) == 16 && per == 8, "the bench shape");
  printf("ok slices\n");
  return true;
}
}  // namespace

int main() {
  if (!(check_weights() && check_lethal() && check_cells() && check_map_order() && check_slices())) return 1;
  printf("ok erpl_casualty_check\n");
  return 0;
}
