// erpl_bands_w_check — erpl_bands_w.h on the host alone (no HIP, no library): what must hold before a kernel runs anywhere.
//   1. T of q: 1 at q = 0, sum_w at q = 1, and either side of an integer product q * sum_w
//   2. a sum_w above 2^53: every W = 2^Q at m = 4099; the integers exact, every quantile a value of the row, ess = count
//   3. a hand-made table with ties, -0.0 / +0.0, NaN and both infinities against the enumeration of the weighted multiset
//   4. an all-zero weight row: every row empty, integers 0, doubles NaN, K = 0, no refusal
//   5. the admitted-weight rule: 2^Q passes, 2^Q + 1 is refused with its column, in a masked column too, and nothing is written
//   6. the refusals come in the order of the header
// Prints one ok line per part; exit status 1 on the first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "erpl_bands_w.h"

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

char g_text[256];
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_text, sizeof(g_text), fmt, ap);
  va_end(ap);
  return code;
}

erpl_bands_w_spec spec_of(int channels, int nodes) {
  erpl_bands_w_spec s;
  memset(&s, 0, sizeof(s));
  s.n_channels = channels; s.n_nodes = nodes;
  return s;
}

bool same_bits(double a, double b) { return erpl_bits_of(a) == erpl_bits_of(b); }

bool check_target() {
  REQUIRE(erpl_rw_target(0.0, 1000) == 1, "T(0) = %llu", (unsigned long long)erpl_rw_target(0.0, 1000));
  REQUIRE(erpl_rw_target(1.0, 1000) == 1000, "T(1) = %llu", (unsigned long long)erpl_rw_target(1.0, 1000));
  REQUIRE(erpl_rw_target(0.25, 1000) == 250, "T(0.25) = %llu", (unsigned long long)erpl_rw_target(0.25, 1000));
  REQUIRE(erpl_rw_target(nextafter(0.25, 1.0), 1000) == 251, "just above an integer product");
  REQUIRE(erpl_rw_target(nextafter(0.25, 0.0), 1000) == 250, "just below an integer product");
  const uint64_t big = (uint64_t)4099 << 49;     // above 2^53: (double) big is exact here, q * big may round
  REQUIRE(erpl_rw_target(1.0, big) == big && erpl_rw_target(0.0, big) == 1, "T at the ends of a sum above 2^53");
  REQUIRE(erpl_rw_target(0.5, big) == big / 2, "T(0.5) of %llu", (unsigned long long)big);
  printf("ok target\n");
  return true;
}

bool check_big_sum() {
  const int64_t m = 4099;
  const int Q = erpl_rw_q(m);
  REQUIRE(Q == 49, "Q(4099) = %d", Q);
  std::vector<double> x((size_t)m);
  std::vector<int64_t> w((size_t)m, (int64_t)1 << Q);
  for (int64_t i = 0; i < m; ++i) x[(size_t)i] = (double)((i * 2654435761ll) % 4099) - 2000.0;   // a permutation of -2000 .. 2098
  erpl_bands_w_spec s = spec_of(1, 1);
  s.n_q = 3; s.q[0] = 0.0; s.q[1] = 0.5; s.q[2] = 1.0;
  s.n_thresholds[0] = 1; s.threshold[0][0] = 0.0;
  erpl_bands_w_row row;
  erpl_bands_w_result res;
  REQUIRE(erpl_bw_host(s, x.data(), nullptr, w.data(), m, m, &row, &res) == -1, "refused");
  REQUIRE(res.K == Q + 1 && res.max_w == ((int64_t)1 << Q) && res.Q == Q, "K = %d", res.K);
  REQUIRE(row.sum_w == m << Q && row.sum_w > ((int64_t)1 << 53), "sum_w = %lld", (long long)row.sum_w);
  REQUIRE(row.count == m && row.exceed_w[0] == (int64_t)2098 << Q, "exceed_w = %lld", (long long)row.exceed_w[0]);
  REQUIRE(row.quantile[0] == -2000.0 && row.quantile[2] == 2098.0 && row.min == -2000.0 && row.max == 2098.0, "extremes");
  REQUIRE(row.quantile[1] == 49.0, "median = %g", row.quantile[1]);   // rank ceil(4099 / 2) = 2050 of -2000 ..
  REQUIRE(fabs(row.ess - (double)m) <= 1e-9 * (double)m, "ess = %.17g", row.ess);
  REQUIRE(fabs(row.mean - 49.0) <= 1e-9, "mean = %.17g", row.mean);
  printf("ok big_sum\n");
  return true;
}

bool check_table() {
  const double inf = INFINITY;
  const double x[12] = {1.0, -0.0, 0.0, 1.0, NAN, inf, -inf, 2.0, 1.0, -3.0, 0.0, 5.0};
  const int64_t w[12] = {3, 2, 1, 0, 7, 7, 7, 4, 1, 2, 0, 9};
  const uint8_t mask[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
  erpl_bands_w_spec s = spec_of(1, 1);
  s.n_q = 4; s.q[0] = 0.0; s.q[1] = 2.0 / 13.0; s.q[2] = 0.5; s.q[3] = 1.0;
  s.n_thresholds[0] = 2; s.threshold[0][0] = 1.0; s.threshold[0][1] = -0.0;
  erpl_bands_w_row row;
  erpl_bands_w_result res;
  REQUIRE(erpl_bw_host(s, x, mask, w, 12, 12, &row, &res) == -1, "refused");
  // members: 1 (3), -0 (2), +0 (1), 2 (4), 1 (1), -3 (2): the multiset -3 -3 -0 -0 +0 1 1 1 1 2 2 2 2, 13 units
  REQUIRE(res.n_masked == 1 && res.n_counted == 11 && res.max_w == 9 && res.K == 4, "call record: K = %d", res.K);
  REQUIRE(row.count == 6 && row.n_non_finite == 3 && row.n_zero == 2 && row.sum_w == 13, "counts %lld %lld %lld %lld",
          (long long)row.count, (long long)row.n_non_finite, (long long)row.n_zero, (long long)row.sum_w);
  std::vector<double> multi;
  for (int i = 0; i < 11; ++i)
    if (erpl_is_finite(x[i])) for (int64_t k = 0; k < w[i]; ++k) multi.push_back(x[i]);
  std::stable_sort(multi.begin(), multi.end(), [](double a, double b) { return erpl_tally_key(a) < erpl_tally_key(b); });
  for (int k = 0; k < 4; ++k) {
    const uint64_t T = erpl_rw_target(s.q[k], 13);
    REQUIRE(same_bits(row.quantile[k], multi[(size_t)T - 1]), "quantile %d = %g, enumeration %g", k, row.quantile[k], multi[(size_t)T - 1]);
  }
  REQUIRE(same_bits(row.quantile[0], -3.0) && same_bits(row.quantile[2], 1.0) && same_bits(row.quantile[3], 2.0), "q = 0, 0.5, 1");
  REQUIRE(row.exceed_w[0] == 4 && row.exceed_w[1] == 8, "exceed_w = %lld %lld", (long long)row.exceed_w[0], (long long)row.exceed_w[1]);
  REQUIRE(same_bits(row.min, -3.0) && same_bits(row.max, 2.0), "extremes");
  const double mean = (3.0 + 8.0 + 1.0 - 6.0) / 13.0;
  REQUIRE(fabs(row.mean - mean) <= 1e-15, "mean = %.17g", row.mean);
  double var = 0.0, s2 = 0.0;
  for (int i = 0; i < 11; ++i)
    if (erpl_is_finite(x[i])) { var += (double)w[i] * (x[i] - mean) * (x[i] - mean); s2 += (double)(w[i] * w[i]); }
  REQUIRE(fabs(row.var - var / 13.0) <= 1e-14, "var = %.17g", row.var);
  REQUIRE(fabs(row.ess - 169.0 / s2) <= 1e-13, "ess = %.17g", row.ess);
  // a zero extreme keeps its sign whatever the order of the columns
  const double z[2] = {0.0, -0.0};
  const int64_t one[2] = {1, 1};
  erpl_bands_w_spec s0 = spec_of(1, 1);
  REQUIRE(erpl_bw_host(s0, z, nullptr, one, 2, 2, &row, &res) == -1, "refused");
  REQUIRE(same_bits(row.min, -0.0) && same_bits(row.max, 0.0), "zero extremes");
  printf("ok table\n");
  return true;
}

bool check_all_zero() {
  const double x[5] = {1.0, 2.0, NAN, 4.0, 5.0};
  const int64_t w[5] = {0, 0, 0, 0, 0};
  erpl_bands_w_spec s = spec_of(1, 1);
  s.n_q = 1; s.q[0] = 0.5;
  s.n_thresholds[0] = 1; s.threshold[0][0] = 1.5;
  erpl_bands_w_row row;
  erpl_bands_w_result res;
  REQUIRE(erpl_bw_host(s, x, nullptr, w, 5, 5, &row, &res) == -1, "refused");
  REQUIRE(res.K == 0 && res.max_w == 0, "K = %d", res.K);
  REQUIRE(row.count == 0 && row.sum_w == 0 && row.exceed_w[0] == 0 && row.n_zero == 4 && row.n_non_finite == 1, "integers");
  REQUIRE(row.mean != row.mean && row.var != row.var && row.ess != row.ess && row.quantile[0] != row.quantile[0] &&
          row.min != row.min && row.max != row.max && row.mean_se != row.mean_se && row.sum_w2 != row.sum_w2 && row.a2[0] != row.a2[0],
          "doubles of an empty row");
  printf("ok all_zero\n");
  return true;
}

bool check_admitted() {
  const int64_t m = 63;
  const int Q = erpl_rw_q(m);
  REQUIRE(Q == 52, "Q(63) = %d", Q);
  REQUIRE(erpl_rw_q(1) == 52 && erpl_rw_q(1024) == 52 && erpl_rw_q(1025) == 51 && erpl_rw_q(4099) == 49, "Q");
  std::vector<double> x((size_t)m, 1.0);
  std::vector<int64_t> w((size_t)m, 1);
  std::vector<uint8_t> mask((size_t)m, 0);
  w[40] = (int64_t)1 << Q;
  erpl_bands_w_spec s = spec_of(1, 1);
  erpl_bands_w_row row;
  erpl_bands_w_result res;
  REQUIRE(erpl_bw_host(s, x.data(), mask.data(), w.data(), m, m, &row, &res) == -1, "2^Q refused");
  REQUIRE(res.K == Q + 1 && row.sum_w == ((int64_t)1 << Q) + 62, "2^Q: K = %d", res.K);
  w[40] += 1; w[50] = -1; mask[40] = 1;
  memset(&row, 0x5a, sizeof(row));
  memset(&res, 0x5a, sizeof(res));
  REQUIRE(erpl_bw_host(s, x.data(), mask.data(), w.data(), m, m, &row, &res) == 40, "2^Q + 1 in a masked column");
  const unsigned char* p = (const unsigned char*)&row;
  for (size_t k = 0; k < sizeof(row); ++k) REQUIRE(p[k] == 0x5a, "the row record was written");
  p = (const unsigned char*)&res;
  for (size_t k = 0; k < sizeof(res); ++k) REQUIRE(p[k] == 0x5a, "the call record was written");
  w[40] = 1;
  REQUIRE(erpl_bw_host(s, x.data(), mask.data(), w.data(), m, m, &row, &res) == 50, "a negative weight");
  printf("ok admitted\n");
  return true;
}

bool check_refusals() {
  erpl_bands_w_spec s = spec_of(2, 3);
  s.n_q = 1; s.q[0] = 0.5;
  const double v = 0.0;
  const int64_t w = 1;
  erpl_bands_w_row row = {};
  erpl_bands_w_result res = {};
  REQUIRE(erpl_bw_check(nullptr, nullptr, nullptr, nullptr, nullptr, 0, -1, fail) == ERPL_ERR_INVALID && strstr(g_text, "spec"), "%s", g_text);
  erpl_bands_w_spec b = s;
  b.n_channels = 9; b.n_nodes = 0;
  REQUIRE(erpl_bw_check(&b, nullptr, nullptr, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "n_channels"), "%s", g_text);
  b = s; b.n_nodes = 4097; b.n_q = 9;
  REQUIRE(erpl_bw_check(&b, nullptr, nullptr, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "n_nodes"), "%s", g_text);
  b = s; b.n_q = 9; b.q[0] = 2.0;
  REQUIRE(erpl_bw_check(&b, nullptr, nullptr, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "n_q"), "%s", g_text);
  b = s; b.q[0] = NAN; b.n_thresholds[1] = 5;
  REQUIRE(erpl_bw_check(&b, nullptr, nullptr, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "q[0]"), "%s", g_text);
  b = s; b.n_thresholds[1] = 5; b.n_thresholds[0] = 1; b.threshold[0][0] = NAN;
  REQUIRE(erpl_bw_check(&b, nullptr, nullptr, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "n_thresholds[1]"), "%s", g_text);
  b = s; b.n_thresholds[1] = 2; b.threshold[1][1] = NAN;
  REQUIRE(erpl_bw_check(&b, nullptr, nullptr, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "threshold[1][1]"), "%s", g_text);
  REQUIRE(erpl_bw_check(&s, nullptr, nullptr, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "values"), "%s", g_text);
  REQUIRE(erpl_bw_check(&s, &v, nullptr, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "weights"), "%s", g_text);
  REQUIRE(erpl_bw_check(&s, &v, &w, nullptr, nullptr, 0, -1, fail) != 0 && strstr(g_text, "rows"), "%s", g_text);
  REQUIRE(erpl_bw_check(&s, &v, &w, &row, nullptr, 0, -1, fail) != 0 && strstr(g_text, "result"), "%s", g_text);
  REQUIRE(erpl_bw_check(&s, &v, &w, &row, &res, 0, -1, fail) != 0 && strstr(g_text, "m = 0"), "%s", g_text);
  REQUIRE(erpl_bw_check(&s, &v, &w, &row, &res, (int64_t)1 << 31, -1, fail) != 0 && strstr(g_text, "m = "), "%s", g_text);
  REQUIRE(erpl_bw_check(&s, &v, &w, &row, &res, 5, 4, fail) != 0 && strstr(g_text, "ld = 4"), "%s", g_text);
  REQUIRE(erpl_bw_check(&s, &v, &w, &row, &res, 5, 5, fail) == ERPL_OK, "a valid call was refused: %s", g_text);
  printf("ok refusals\n");
  return true;
}
}  // namespace

int main() {
  if (!check_target() || !check_big_sum() || !check_table() || !check_all_zero() || !check_admitted() || !check_refusals()) return 1;
  printf("ok\n");
  return 0;
}
