// erpl_cdrv_check — erpl_cdrv.h on the host alone (no HIP, no library): what must hold before a kernel runs anywhere.
//   1. the product index: the F squares first, then the pairs f < g row by row, every index once
//   2. segments and slices: multiples of 256 / ERPL_CDRV_KT that cover m at m = 1, 255, 256, 257, 4099, 2^20, 2^31 - 1
//   3. sums -> pearson / src / r2 / ok: a table of 5 factors and 9 rows - an ordinary row, an empty one, a population of one, a
//      constant row, a row constant as -0.0 / +0.0, a row whose population makes one factor constant, a row with count = F and
//      one with count < F - through the sums the product pass forms (standardised over the base population, masked) and
//      erpl_cdrv_finish_row, against the two-pass formulae and a Gaussian elimination of the same normal equations
//   4. an affine pair of factors: every row fails the regression, its pearson stays
//   5. the rule that sends a (row, factor) to the exact extremes: never a constant factor past it, at large offsets either
// Prints one ok line per part; exit status 1 on the first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_cdrv.h"

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

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double uniform() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (double)(g_state >> 11) * 0x1p-53;
}

bool check_index() {
  for (int F = 1; F <= ERPL_CDRV_MAX_FACTORS; ++F) {
    const int P = erpl_cdrv_products(F, true);
    REQUIRE(P == F * (F + 1) / 2 && erpl_cdrv_products(F, false) == F, "the product count of F = %d", F);
    std::vector<int> seen((size_t)P, 0);
    int next = F;
    for (int f = 0; f < F; ++f) {
      REQUIRE(erpl_cdrv_product_index(F, f, f) == f, "the square of factor %d of %d", f, F);
      ++seen[(size_t)f];
      for (int g = f + 1; g < F; ++g) {
        const int p = erpl_cdrv_product_index(F, f, g);
        REQUIRE(p == next && p < P, "pair (%d, %d) of %d at %d, not %d", f, g, F, p, next);
        ++seen[(size_t)p];
        ++next;
      }
    }
    for (int p = 0; p < P; ++p) REQUIRE(seen[(size_t)p] == 1, "index %d of F = %d met %d times", p, F, seen[(size_t)p]);
    REQUIRE(erpl_cdrv_row_doubles(F, true) % 4 == 0 && erpl_cdrv_row_doubles(F, true) > 2 * ERPL_CDRV_LIN + 16 * erpl_cdrv_product_blocks(F, true),
            "the record of F = %d", F);
  }
  REQUIRE(ERPL_CDRV_ONE >= ERPL_CDRV_MAX_FACTORS && ERPL_CDRV_ZERO > ERPL_CDRV_ONE && ERPL_CDRV_ZERO < ERPL_CDRV_LIN, "the linear columns");
  printf("ok product index\n");
  return true;
}

bool check_cuts() {
  const int64_t ms[7] = {1, 255, 256, 257, 4099, 1 << 20, 2147483647ll};
  for (int64_t m : ms) {
    int64_t seg = 0, slice = 0;
    const int segs = erpl_cdrv_segments(m, &seg), slices = erpl_cdrv_slices(m, &slice);
    REQUIRE(segs >= 1 && segs <= ERPL_CDRV_MAX_SEGS && seg % 256 == 0 && (int64_t)segs * seg >= m && (int64_t)(segs - 1) * seg < m,
            "m = %lld: %d segments of %lld", (long long)m, segs, (long long)seg);
    REQUIRE(slices >= 1 && slices <= ERPL_CDRV_MAX_SLICES && slice % ERPL_CDRV_KT == 0 && (int64_t)slices * slice >= m &&
            (int64_t)(slices - 1) * slice < m, "m = %lld: %d slices of %lld", (long long)m, slices, (long long)slice);
    REQUIRE(erpl_cdrv_chunk_tiles(m, 32, true) >= 1, "m = %lld: no tile fits a launch", (long long)m);
  }
  printf("ok segments and slices\n");
  return true;
}

// the table of parts 3 and 4
struct Table {
  int F, R, m;
  std::vector<double> x, y;        // [F][m], [R][m]
  std::vector<uint8_t> mask;       // [m]
  double fx(int f, int i) const { return x[(size_t)f * m + i]; }
  double fy(int r, int i) const { return y[(size_t)r * m + i]; }
};

Table make_table(bool affine) {
  Table t;
  t.F = 5; t.R = 9; t.m = 301;
  t.x.assign((size_t)t.F * t.m, 0.0);
  t.y.assign((size_t)t.R * t.m, NAN);
  t.mask.assign((size_t)t.m, 0);
  for (int i = 0; i < t.m; ++i) {
    t.mask[(size_t)i] = i % 10 == 3 ? 4 : 0;
    for (int f = 0; f < t.F; ++f) t.x[(size_t)f * t.m + i] = 1e4 * (f + 1) + (f + 1) * (uniform() - 0.5);
    t.x[(size_t)2 * t.m + i] = 7.0 + 0.57 * (t.fx(0, i) - 1e4) + 0.8 * (uniform() - 0.5);   // correlated with factor 0
    t.x[(size_t)4 * t.m + i] = i < 40 ? 2.5 : 2.5 + uniform();                                // constant on the first 40 columns
    if (affine) t.x[(size_t)3 * t.m + i] = 3.0 - 2.0 * t.fx(1, i);
    if (i == 17) t.x[(size_t)1 * t.m + i] = NAN;
  }
  for (int i = 0; i < t.m; ++i) {
    double lin = 0.0;
    for (int f = 0; f < t.F; ++f) lin += (f % 2 ? -1.0 : 1.0) * (f + 1) * t.fx(f, i);
    if (i % 3 != 1) t.y[(size_t)0 * t.m + i] = lin + 0.3 * uniform();        // 0: ordinary, a third missing
    /* 1: empty */
    if (i == 55) t.y[(size_t)2 * t.m + i] = 1.25;                           // 2: a population of one
    if (i % 2) t.y[(size_t)3 * t.m + i] = -3.5;                             // 3: constant
    if (i % 2 == 0) t.y[(size_t)4 * t.m + i] = i % 4 ? 0.0 : -0.0;          // 4: constant as -0.0 / +0.0
    if (i < 40) t.y[(size_t)5 * t.m + i] = lin * lin * 1e-9 + uniform();    // 5: factor 4 is constant on this population
    if (i >= 100 && i < 100 + 6) t.y[(size_t)6 * t.m + i] = uniform();      // 6: count = F (one of the six is masked)
    if (i >= 200 && i < 200 + 3) t.y[(size_t)7 * t.m + i] = uniform();      // 7: count < F
    t.y[(size_t)8 * t.m + i] = i % 7 == 0 ? INFINITY : lin - 2.0 * uniform();   // 8: infinities
  }
  return t;
}

// Gaussian elimination with partial pivoting of the k x k system A z = b (both overwritten); false: singular to working precision
bool solve(std::vector<double>& A, std::vector<double>& b, int k) {
  for (int c = 0; c < k; ++c) {
    int piv = c;
    for (int r = c + 1; r < k; ++r) if (fabs(A[(size_t)r * k + c]) > fabs(A[(size_t)piv * k + c])) piv = r;
    if (fabs(A[(size_t)piv * k + c]) < 1e-12) return false;
    for (int j = 0; j < k; ++j) std::swap(A[(size_t)c * k + j], A[(size_t)piv * k + j]);
    std::swap(b[(size_t)c], b[(size_t)piv]);
    for (int r = c + 1; r < k; ++r) {
      const double w = A[(size_t)r * k + c] / A[(size_t)c * k + c];
      for (int j = c; j < k; ++j) A[(size_t)r * k + j] -= w * A[(size_t)c * k + j];
      b[(size_t)r] -= w * b[(size_t)c];
    }
  }
  for (int c = k - 1; c >= 0; --c) {
    for (int j = c + 1; j < k; ++j) b[(size_t)c] -= A[(size_t)c * k + j] * b[(size_t)j];
    b[(size_t)c] /= A[(size_t)c * k + c];
  }
  return true;
}

bool check_table(bool affine) {
  const Table t = make_table(affine);
  const int F = t.F, m = t.m;
  // the base population and the factors over it
  std::vector<uint8_t> base((size_t)m);
  double fmean[5] = {}, fstd[5] = {}, fmin[5], fmax[5];
  int n_base = 0;
  for (int i = 0; i < m; ++i) {
    bool ok = t.mask[(size_t)i] == 0;
    for (int f = 0; f < F; ++f) ok = ok && std::isfinite(t.fx(f, i));
    base[(size_t)i] = ok ? 0 : 1;
    n_base += ok;
  }
  for (int f = 0; f < F; ++f) {
    fmin[f] = INFINITY; fmax[f] = -INFINITY;
    for (int i = 0; i < m; ++i) if (!base[(size_t)i]) { fmean[f] += t.fx(f, i); fmin[f] = std::min(fmin[f], t.fx(f, i)); fmax[f] = std::max(fmax[f], t.fx(f, i)); }
    fmean[f] /= n_base;
    for (int i = 0; i < m; ++i) if (!base[(size_t)i]) fstd[f] += (t.fx(f, i) - fmean[f]) * (t.fx(f, i) - fmean[f]);
    fstd[f] = sqrt(fstd[f] / n_base);
  }
  const int rd = erpl_cdrv_row_doubles(F, true), nc = 16 * erpl_cdrv_product_blocks(F, true);
  for (int r = 0; r < t.R; ++r) {
    // the row over its own population, two passes
    std::vector<int> pop;
    for (int i = 0; i < m; ++i) if (!base[(size_t)i] && std::isfinite(t.fy(r, i))) pop.push_back(i);
    const int64_t count = (int64_t)pop.size();
    double ymean = 0.0, ystd = 0.0, ymin = INFINITY, ymax = -INFINITY;
    for (int i : pop) { ymean += t.fy(r, i); ymin = std::min(ymin, t.fy(r, i)); ymax = std::max(ymax, t.fy(r, i)); }
    ymean /= (double)count;
    for (int i : pop) ystd += (t.fy(r, i) - ymean) * (t.fy(r, i) - ymean);
    ystd = sqrt(ystd / (double)count);
    const bool row_constant = count > 0 && ymin == ymax;
    const double yinv = ystd > 0.0 ? 1.0 / ystd : 0.0;
    // the sums as the product pass forms them
    std::vector<double> rec((size_t)rd, 0.0);
    int32_t fconst[5];
    for (int f = 0; f < F; ++f) {
      double lo = INFINITY, hi = -INFINITY;
      for (int i : pop) { lo = std::min(lo, t.fx(f, i)); hi = std::max(hi, t.fx(f, i)); }
      fconst[f] = count > 0 && lo == hi ? 1 : 0;
    }
    for (int i : pop) {
      double xs[5];
      const double ys = (t.fy(r, i) - ymean) * yinv;
      for (int f = 0; f < F; ++f) xs[f] = (t.fx(f, i) - fmean[f]) * (1.0 / fstd[f]);
      rec[ERPL_CDRV_ONE] += 1.0;
      rec[(size_t)(ERPL_CDRV_LIN + nc + ERPL_CDRV_ONE)] += ys;
      rec[(size_t)(2 * ERPL_CDRV_LIN + nc)] += ys * ys;
      for (int f = 0; f < F; ++f) {
        rec[(size_t)f] += xs[f];
        rec[(size_t)(ERPL_CDRV_LIN + nc + f)] += ys * xs[f];
        for (int g = f; g < F; ++g) rec[(size_t)(ERPL_CDRV_LIN + erpl_cdrv_product_index(F, f, g))] += xs[f] * xs[g];
      }
    }
    const ErplCdrvRowView v = erpl_cdrv_row_view(rec.data(), F, true);
    REQUIRE(v.n1 == (double)count, "row %d: the count among the sums", r);
    for (int f = 0; f < F; ++f)
      if (count >= 2 && fconst[f]) REQUIRE(erpl_cdrv_ambiguous(v.c[f], v.a[f], (double)count), "row %d: constant factor %d passes as proven", r, f);
    double pearson[5], src[5], r2, pivot;
    int32_t ok;
    erpl_cdrv_finish_row(F, true, count, row_constant, fconst, v, pearson, src, &r2, &pivot, &ok);
    // the two-pass formulae
    std::vector<int> use;
    std::vector<double> sxx((size_t)F, 0.0), sxy((size_t)F, 0.0), xm((size_t)F, 0.0);
    double syy = 0.0;
    for (int f = 0; f < F; ++f) { for (int i : pop) xm[(size_t)f] += t.fx(f, i); xm[(size_t)f] /= (double)count; }
    for (int i : pop) {
      syy += (t.fy(r, i) - ymean) * (t.fy(r, i) - ymean);
      for (int f = 0; f < F; ++f) {
        sxx[(size_t)f] += (t.fx(f, i) - xm[(size_t)f]) * (t.fx(f, i) - xm[(size_t)f]);
        sxy[(size_t)f] += (t.fx(f, i) - xm[(size_t)f]) * (t.fy(r, i) - ymean);
      }
    }
    for (int f = 0; f < F; ++f) {
      const bool want_nan = count < 2 || row_constant || fconst[f];
      if (want_nan) {
        REQUIRE(pearson[f] != pearson[f], "row %d factor %d: pearson %g where the contract says NaN", r, f, pearson[f]);
      } else {
        const double want = sxy[(size_t)f] / sqrt(sxx[(size_t)f] * syy);
        REQUIRE(fabs(pearson[f] - want) <= 1e-12, "row %d factor %d: pearson %.17g, two passes give %.17g", r, f, pearson[f], want);
        use.push_back(f);
      }
    }
    const int k = (int)use.size();
    const bool too_few = count <= k;   // the correlation matrix of k factors over at most k points is singular
    if (count < 2) {
      REQUIRE(!ok && pivot != pivot && r2 != r2, "row %d: a regression over fewer than two points", r);
      continue;
    }
    if (affine || too_few) {
      REQUIRE(!ok && r2 != r2 && pivot == pivot && !(pivot >= 1e-10), "row %d: ok = %d, pivot %g, r2 %g of a singular regression", r, ok, pivot, r2);
      for (int f = 0; f < F; ++f) REQUIRE(src[f] != src[f], "row %d factor %d: src %g of a failed regression", r, f, src[f]);
      continue;
    }
    if (row_constant) {
      REQUIRE(r2 != r2, "row %d: r2 %g of a constant row", r, r2);
      for (int f = 0; f < F; ++f) REQUIRE(src[f] != src[f], "row %d factor %d: src %g of a constant row", r, f, src[f]);
      continue;
    }
    REQUIRE(ok && pivot >= 1e-10 && pivot <= 1.0 + 1e-12, "row %d: ok = %d, pivot %g", r, ok, pivot);
    // the normal equations of the standardised regression, solved another way
    std::vector<double> A((size_t)k * k), b((size_t)k);
    for (int p = 0; p < k; ++p) {
      b[(size_t)p] = sxy[(size_t)use[(size_t)p]] / sqrt(sxx[(size_t)use[(size_t)p]] * syy);
      for (int q = 0; q < k; ++q) {
        double s = 0.0;
        for (int i : pop) s += (t.fx(use[(size_t)p], i) - xm[(size_t)use[(size_t)p]]) * (t.fx(use[(size_t)q], i) - xm[(size_t)use[(size_t)q]]);
        A[(size_t)p * k + q] = s / sqrt(sxx[(size_t)use[(size_t)p]] * sxx[(size_t)use[(size_t)q]]);
      }
    }
    const std::vector<double> rfy = b;
    REQUIRE(solve(A, b, k), "row %d: the check's own elimination failed", r);
    double fit = 0.0;
    for (int p = 0; p < k; ++p) {
      REQUIRE(fabs(src[use[(size_t)p]] - b[(size_t)p]) <= 1e-10, "row %d factor %d: src %.17g, elimination gives %.17g", r, use[(size_t)p], src[use[(size_t)p]], b[(size_t)p]);
      fit += b[(size_t)p] * rfy[(size_t)p];
    }
    for (int f = 0; f < F; ++f) if (fconst[f]) REQUIRE(src[f] != src[f], "row %d: src %g of the constant factor %d", r, src[f], f);
    REQUIRE(fabs(r2 - fit) <= 1e-10 && r2 > -1e-10 && r2 < 1.0 + 1e-10, "row %d: r2 %.17g, elimination gives %.17g", r, r2, fit);
  }
  printf(affine ? "ok affine pair\n" : "ok rows\n");
  return true;
}

bool check_ambiguous() {
  // constant values, far from zero in standardised units, summed in the worst order: never proven non-constant
  const double offsets[5] = {0.0, 1.0, -37.25, 1e4 / 3.0, 1e6 * 0.7};
  const int counts[4] = {2, 3, 1000, 1 << 20};
  for (double c : offsets)
    for (int n : counts) {
      double s1 = 0.0, s2 = 0.0;
      for (int i = 0; i < n; ++i) { s1 += c; s2 += c * c; }
      REQUIRE(erpl_cdrv_ambiguous(s2, s1, (double)n), "a constant %g over %d columns passes as proven", c, n);
    }
  // standardised values of unit spread about a moderate offset: proven
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < 1000; ++i) { const double x = 3.0 + 2.0 * (uniform() - 0.5); s1 += x; s2 += x * x; }
  REQUIRE(!erpl_cdrv_ambiguous(s2, s1, 1000.0), "an ordinary factor is sent to the extremes");
  printf("ok extremes rule\n");
  return true;
}
}  // namespace

int main() {
  if (!(check_index() && check_cuts() && check_table(false) && check_table(true) && check_ambiguous())) return 1;
  printf("ok erpl_cdrv_check\n");
  return 0;
}
