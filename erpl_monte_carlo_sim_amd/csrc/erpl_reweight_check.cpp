// erpl_reweight_check — erpl_reweight.h on the host alone (no HIP, no library): what must hold before a kernel runs anywhere.
//   1. the portable exp: 1 at 0, positive at -64 and 0 just below it (and for a NaN), never above 1; at every boundary between
//      two values of k (x = (k + 1/2) ln 2, k = -1 .. -92) and one double either side of it within 2 ulp of libm's exp, the
//      value below the boundary not above the one above it
//   2. W is monotone in l on a grid of 2^-10 over [-70, 0]; 2^Q at l = l_max, 0 more than 64 below it
//   3. an identity law (normal rows mu 0, s 1, uniform rows (0, 1)) gives every W = 2^Q, ess = count, sum_w = count 2^Q
//   4. a window of columns gives the log-weights of those columns of the whole, bit for bit
//   5. the weighted rank rule on a hand-made table with ties, zero weights and zeros of both signs, and T of q
// Prints one ok line per part; exit status 1 on the first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_reweight.h"

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

double ulps(double got, double want) { return fabs(got - want) / (nextafter(want, INFINITY) - want); }

// a fixed table: uniforms in (0, 1) from a 64-bit LCG, normals as a sum of twelve of them minus 6
struct Lcg {
  uint64_t s;
  double u() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(s >> 11) + 0.5) * 0x1p-53;
  }
  double z() {
    double a = 0.0;
    for (int k = 0; k < 12; ++k) a += u();
    return a - 6.0;
  }
};

bool check_exp() {
  REQUIRE(erpl_rw_exp(0.0) == 1.0 && erpl_rw_exp(-0.0) == 1.0, "exp(0) = %.17g", erpl_rw_exp(0.0));
  REQUIRE(erpl_rw_exp(-64.0) > 0.0 && ulps(erpl_rw_exp(-64.0), exp(-64.0)) <= 2.0, "exp(-64) = %.17g", erpl_rw_exp(-64.0));
  REQUIRE(erpl_rw_exp(nextafter(-64.0, -INFINITY)) == 0.0 && erpl_rw_exp(-1e300) == 0.0 && erpl_rw_exp(-INFINITY) == 0.0, "below -64");
  REQUIRE(erpl_rw_exp(NAN) == 0.0, "exp(NaN) = %.17g", erpl_rw_exp(NAN));
  double worst = 0.0;
  for (int k = -1; k >= -92; --k) {
    const double edge = ((double)k + 0.5) * 0.6931471805599453;
    const double x[3] = {nextafter(edge, -INFINITY), edge, nextafter(edge, INFINITY)};
    double v[3];
    for (int j = 0; j < 3; ++j) {
      v[j] = erpl_rw_exp(x[j]);
      const double e = ulps(v[j], exp(x[j]));
      worst = e > worst ? e : worst;
      REQUIRE(e <= 2.0 && v[j] <= 1.0 && v[j] > 0.0, "k = %d: exp(%.17g) = %.17g, %.2f ulp from libm", k, x[j], v[j], e);
    }
    REQUIRE(v[0] <= v[2], "k = %d: %.17g above %.17g across the boundary", k, v[0], v[2]);
  }
  for (double x = -64.0; x <= 0.0; x += 0x1p-12) REQUIRE(erpl_rw_exp(x) <= 1.0, "exp(%.17g) exceeds 1", x);
  printf("ok exp: at most %.2f ulp from libm at the k boundaries\n", worst);
  return true;
}

bool check_monotone() {
  const int Q = erpl_rw_q(1000);
  REQUIRE(Q == 52 && erpl_rw_q(1) == 52 && erpl_rw_q(1024) == 52 && erpl_rw_q(1025) == 51 && erpl_rw_q(((int64_t)1 << 31) - 1) == 31,
          "Q of n: %d %d %d %d", Q, erpl_rw_q(1024), erpl_rw_q(1025), erpl_rw_q(((int64_t)1 << 31) - 1));
  const double lmax = 3.25;
  int64_t before = 0;
  for (double d = -70.0; d <= 0.0; d += 0x1p-10) {
    const int64_t w = erpl_rw_weight(lmax + d, lmax, Q);
    REQUIRE(w >= before && w >= 0, "W falls from %lld to %lld at l - l_max = %.17g", (long long)before, (long long)w, d);
    if (d < -64.0) REQUIRE(w == 0, "W = %lld at l - l_max = %.17g", (long long)w, d);
    before = w;
  }
  REQUIRE(before == (int64_t)1 << Q, "the heaviest W = %lld", (long long)before);
  printf("ok monotone\n");
  return true;
}

// four law rows (normal, uniform, normal, uniform) and a summary of n columns, ld columns apart
struct Table {
  int64_t n, ld;
  std::vector<double> factors, summary;
  Table(int64_t n_, int64_t ld_, uint64_t seed) : n(n_), ld(ld_), factors((size_t)(4 * ld_), -7.0), summary((size_t)(ERPL_SUMMARY_DIM * ld_), -7.0) {
    Lcg g = {seed};
    for (int64_t i = 0; i < n; ++i) {
      for (int r = 0; r < 4; ++r) factors[(size_t)(r * ld + i)] = (r & 1) ? g.u() : g.z();
      for (int r = 0; r < ERPL_SUMMARY_DIM; ++r) summary[(size_t)(r * ld + i)] = 100.0 * g.z() + r;
    }
  }
};

erpl_rw_spec four_rows() {
  erpl_rw_spec sp = {};
  sp.n_law = 4;
  for (int r = 0; r < 4; ++r) {
    sp.kind[r] = (r & 1) ? ERPL_DESIGN_UNIFORM : ERPL_DESIGN_NORMAL;
    sp.mu[r] = 0.0; sp.s[r] = 1.0; sp.a[r] = 0.0; sp.b[r] = 1.0;
  }
  sp.n_rows = 2; sp.rows[0] = ERPL_SUM_APOGEE_ALT; sp.rows[1] = ERPL_SUM_RANGE;
  sp.n_thresholds[0] = 1; sp.threshold[0][0] = 0.0;
  sp.n_q = 3; sp.q[0] = 0.0; sp.q[1] = 0.5; sp.q[2] = 1.0;
  return sp;
}

bool check_identity() {
  const int64_t n = 1500;
  Table t(n, n + 5, 7);
  const erpl_rw_spec sp = four_rows();
  erpl_reweight res;
  std::vector<double> logw((size_t)n);
  std::vector<int64_t> w((size_t)n);
  erpl_rw_host(sp, t.factors.data(), t.ld, t.summary.data(), t.ld, nullptr, nullptr, n, &res, logw.data(), w.data());
  const int Q = erpl_rw_q(n);
  REQUIRE(Q == 51 && res.Q == Q && res.count == n && res.n_zero == 0 && res.n_outside == 0, "Q = %d, count = %lld", res.Q, (long long)res.count);
  for (int64_t i = 0; i < n; ++i)
    REQUIRE(logw[(size_t)i] == 0.0 && w[(size_t)i] == (int64_t)1 << Q, "column %lld: l = %.17g, W = %lld", (long long)i, logw[(size_t)i], (long long)w[(size_t)i]);
  REQUIRE(res.sum_w == n << Q && res.max_w == (int64_t)1 << Q && res.ess == (double)n, "sum_w = %lld, ess = %.17g", (long long)res.sum_w, res.ess);
  REQUIRE(res.ess_expected_share == 1.0, "share = %.17g", res.ess_expected_share);
  const double* x = &t.summary[(size_t)(ERPL_SUM_APOGEE_ALT * t.ld)];
  double mn = x[0], mx = x[0];
  int64_t above = 0;
  for (int64_t i = 0; i < n; ++i) { mn = x[i] < mn ? x[i] : mn; mx = x[i] > mx ? x[i] : mx; above += x[i] > 0.0; }
  REQUIRE(res.row[0].quantile[0] == mn && res.row[0].quantile[2] == mx && res.row[0].min == mn && res.row[0].max == mx, "extremes");
  REQUIRE(res.row[0].exceed_w[0] == above << Q && res.row[0].p[0] == (double)above / (double)n, "exceedance");
  printf("ok identity\n");
  return true;
}

bool check_windows() {
  const int64_t n = 701, first = 37, count = 129;
  Table t(n, n + 3, 11);
  erpl_rw_spec sp = four_rows();
  sp.mu[0] = 0.3; sp.s[0] = 0.7; sp.a[1] = 0.2; sp.b[1] = 0.6; sp.mu[2] = -0.2; sp.s[2] = 1.1; sp.a[3] = 0.0; sp.b[3] = 0.9;
  t.factors[(size_t)(2 * t.ld + first + 3)] = NAN;
  std::vector<uint8_t> mask((size_t)n, 0);
  mask[(size_t)(first + 5)] = 1;
  erpl_reweight whole, win;
  std::vector<double> l_whole((size_t)n), l_win((size_t)count);
  erpl_rw_host(sp, t.factors.data(), t.ld, t.summary.data(), t.ld, nullptr, mask.data(), n, &whole, l_whole.data(), nullptr);
  erpl_rw_host(sp, t.factors.data() + first, t.ld, t.summary.data() + first, t.ld, nullptr, mask.data() + first, count, &win, l_win.data(),
               nullptr);
  REQUIRE(memcmp(l_win.data(), &l_whole[(size_t)first], (size_t)count * sizeof(double)) == 0, "the window's log-weights differ from the whole's");
  REQUIRE(whole.n_masked == 1 && whole.n_non_finite == 1 && whole.n_outside > 0 && whole.count > 0 &&
              whole.n_masked + whole.n_non_finite + whole.n_outside + whole.count == n, "the counts of the whole");
  REQUIRE(l_whole[(size_t)(first + 5)] != l_whole[(size_t)(first + 5)] && l_whole[(size_t)(first + 3)] != l_whole[(size_t)(first + 3)], "NaN where masked / non-finite");
  printf("ok windows: %lld of %lld columns in the support\n", (long long)whole.count, (long long)n);
  return true;
}

bool check_ranks() {
  const double x[7] = {0.0, -0.0, 1.0, 1.0, -1.0, 0.0, 2.0};
  const int64_t w[7] = {2, 3, 0, 4, 1, 0, 5};   // ascending: -1 (1), -0 (3), +0 (2), 1 (4), 2 (5): 15 units
  const double want[15] = {-1.0, -0.0, -0.0, -0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0};
  for (uint64_t T = 1; T <= 15; ++T) {
    uint64_t key = 0;
    erpl_rw_select_host(x, w, 7, &T, 1, &key);
    const double v = erpl_double_of(erpl_tally_bits_of_key(key));
    REQUIRE(erpl_bits_of(v) == erpl_bits_of(want[T - 1]), "T = %llu: %.17g (sign %d)", (unsigned long long)T, v, (int)signbit(v));
  }
  REQUIRE(erpl_rw_target(0.0, 15) == 1 && erpl_rw_target(1.0, 15) == 15 && erpl_rw_target(0.5, 15) == 8 && erpl_rw_target(0.2, 15) == 3, "T of q");
  REQUIRE(erpl_rw_target(1.0, 1ull << 62) == 1ull << 62 && erpl_rw_target(1.0, (1ull << 62) - 1) == (1ull << 62) - 1 && erpl_rw_target(0.5, 1) == 1,
          "T of q at the ends");
  printf("ok ranks\n");
  return true;
}
}  // namespace

int main() {
  if (!(check_exp() && check_monotone() && check_identity() && check_windows() && check_ranks())) return 1;
  printf("ok erpl_reweight_check\n");
  return 0;
}
