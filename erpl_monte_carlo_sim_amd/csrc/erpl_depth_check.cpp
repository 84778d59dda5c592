// erpl_depth_check — erpl_depth.h on the host alone (no HIP, no library): what must hold before a kernel runs anywhere.
//   1. cov = C2(n) - C2(a) - C2(b) against the enumeration of the pairs (pairs with the member itself included) whose band
//      contains the member, on small tables with ties, zeros of both signs and holes; the two terms of a node
//   2. h: central = 1 gives n, central = 1 / n gives 1, a product just below / at / just above an integer, the clamps
//   3. the fences: one rounding per operation, factor = 0 gives the envelope, an overflowing width gives infinite fences
//   4. the path of the rank pass at the built-in limit and under lds_limit; keys and threads of an LDS workgroup
//   5. the pieces of the workspace: aligned, disjoint, `need` their end, no overflow at the shape limits
// Prints one ok line per part; exit status 1 on the first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_depth.h"

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
uint64_t next_u64() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return g_state;
}

bool check_cov() {
  REQUIRE(erpl_depth_c2(0) == 0 && erpl_depth_c2(1) == 0 && erpl_depth_c2(2) == 1 && erpl_depth_c2(5) == 10, "C2 of small n");
  REQUIRE(erpl_depth_c2(2147483647LL) == 2305843005992468481LL, "C2 at the largest m");
  for (int trial = 0; trial < 200; ++trial) {
    const int m = 1 + (int)(next_u64() % 12);
    std::vector<double> x((size_t)m);
    std::vector<int> in((size_t)m);
    int n = 0;
    for (int j = 0; j < m; ++j) {
      const int v = (int)(next_u64() % 5) - 2;   // heavy ties
      x[(size_t)j] = v == 0 ? ((next_u64() & 1) ? -0.0 : 0.0) : (double)v;
      in[(size_t)j] = (next_u64() % 5) != 0;     // a hole in one of five
      n += in[(size_t)j];
    }
    for (int j = 0; j < m; ++j) {
      if (!in[(size_t)j]) continue;
      int a = 0, b = 0;
      for (int i = 0; i < m; ++i) {
        if (!in[(size_t)i]) continue;
        a += x[(size_t)i] < x[(size_t)j];
        b += x[(size_t)i] > x[(size_t)j];
      }
      int64_t pairs = 0;   // {p, q}, p < q, both members, min <= x_j <= max
      for (int p = 0; p < m; ++p)
        for (int q = p + 1; q < m; ++q) {
          if (!in[(size_t)p] || !in[(size_t)q]) continue;
          const double lo = x[(size_t)p] < x[(size_t)q] ? x[(size_t)p] : x[(size_t)q];
          const double hi = x[(size_t)p] > x[(size_t)q] ? x[(size_t)p] : x[(size_t)q];
          pairs += lo <= x[(size_t)j] && x[(size_t)j] <= hi;
        }
      REQUIRE(erpl_depth_cov(n, a, b) == pairs, "trial %d column %d: cov %lld, %lld pairs", trial, j, (long long)erpl_depth_cov(n, a, b),
              (long long)pairs);
      if (n >= 2) {
        const double t = erpl_depth_term(n, a, b), e = erpl_depth_mei_term(n, a);
        REQUIRE(t == (double)pairs / (double)(n * (n - 1) / 2) && t > 0.0 && t <= 1.0, "trial %d column %d: term %g", trial, j, t);
        REQUIRE(e == (double)(n - a) / (double)n && e > 0.0 && e <= 1.0, "trial %d column %d: mei term %g", trial, j, e);
      }
    }
  }
  // the extremes of a row without ties: n - 1 pairs hold them; its middle member of an odd row: every pair but the one-sided ones
  REQUIRE(erpl_depth_cov(9, 0, 8) == 8 && erpl_depth_cov(9, 8, 0) == 8 && erpl_depth_cov(9, 4, 4) == 36 - 12, "cov of an untied row");
  REQUIRE(erpl_depth_cov(7, 0, 0) == 21, "a row of one repeated value: every pair holds every member");
  const int64_t big = 2147483647LL;
  REQUIRE(erpl_depth_cov(big, big - 1, 0) == big - 1 && erpl_depth_cov(big, 0, 0) == erpl_depth_c2(big), "cov at the largest m");
  printf("ok cov\n");
  return true;
}

bool check_h() {
  REQUIRE(erpl_depth_h(0.5, 0) == 0 && erpl_depth_h(1.0, 0) == 0, "nothing defined");
  for (int64_t n : {1LL, 2LL, 3LL, 7LL, 10LL, 400LL, 4099LL, 1048576LL, 2147483647LL}) {
    REQUIRE(erpl_depth_h(1.0, n) == n, "central = 1 at n = %lld", (long long)n);
    // (1 / n) n lies within half an ulp of 1 and rounds to 1 or to its lower neighbour: the ceiling is 1
    REQUIRE(erpl_depth_h(1.0 / (double)n, n) == 1, "central = 1 / n at n = %lld", (long long)n);
    REQUIRE(erpl_depth_h(1e-300, n) == 1, "the lower clamp at n = %lld", (long long)n);
    const int64_t h = erpl_depth_h(0.5, n);
    REQUIRE(h == (n + 1) / 2, "central = 0.5 at n = %lld: %lld", (long long)n, (long long)h);
  }
  // just either side of an integer product: 0.25 * 8 = 2 exactly; the neighbours of 0.25 give 2 and 3
  REQUIRE(erpl_depth_h(0.25, 8) == 2, "an exact product");
  REQUIRE(erpl_depth_h(nextafter(0.25, 0.0), 8) == 2, "a product just below an integer");
  REQUIRE(erpl_depth_h(nextafter(0.25, 1.0), 8) == 3, "a product just above an integer");
  REQUIRE(erpl_depth_h(nextafter(1.0, 0.0), 8) == 8 && erpl_depth_h(nextafter(1.0, 0.0), 1) == 1, "central just below 1");
  printf("ok h\n");
  return true;
}

bool check_fences() {
  double lo, hi;
  erpl_depth_fences(1.0, 3.0, 1.5, &lo, &hi);
  REQUIRE(lo == -2.0 && hi == 6.0, "the fences of [1, 3] at 1.5: %g %g", lo, hi);
  erpl_depth_fences(-0.7, 0.1, 0.0, &lo, &hi);
  REQUIRE(lo == -0.7 && hi == 0.1, "factor 0 gives the envelope");
  const double a = 0.1, b = 0.7, f = 1.3;
  erpl_depth_fences(a, b, f, &lo, &hi);
  volatile double w = b - a;
  volatile double reach = f * w;
  REQUIRE(lo == a - reach && hi == b + reach, "one rounding per operation");
  erpl_depth_fences(-1.7e308, 1.7e308, 1.5, &lo, &hi);
  REQUIRE(std::isinf(lo) && lo < 0 && std::isinf(hi) && hi > 0, "an overflowing width gives infinite fences");
  erpl_depth_fences(5.0, 5.0, 1.5, &lo, &hi);
  REQUIRE(lo == 5.0 && hi == 5.0, "an envelope of one value");
  printf("ok fences\n");
  return true;
}

bool check_path() {
  const int64_t L = ERPL_DEPTH_LDS_MAX;
  REQUIRE(erpl_depth_use_lds(1, 0) && erpl_depth_use_lds(L, 0) && !erpl_depth_use_lds(L + 1, 0), "the built-in limit");
  REQUIRE(erpl_depth_use_lds(16, 16) && !erpl_depth_use_lds(17, 16) && erpl_depth_use_lds(1, 1) && !erpl_depth_use_lds(2, 1), "lds_limit");
  REQUIRE(erpl_depth_lds_limit(2147483647) == L && erpl_depth_use_lds(L, (int32_t)L + 1) && !erpl_depth_use_lds(L + 1, 2147483647),
          "lds_limit is clamped to the built-in limit");
  for (int64_t m = 1; m <= L; m += (m < 300 ? 1 : 97)) {
    const int keys = erpl_depth_lds_keys(m), threads = erpl_depth_lds_threads(m);
    REQUIRE(keys >= m && (keys & (keys - 1)) == 0 && (keys < 2 * m || keys == 2 * ERPL_DEPTH_LDS_MIN_THREADS), "keys of m = %lld", (long long)m);
    REQUIRE(threads >= ERPL_DEPTH_LDS_MIN_THREADS && threads <= ERPL_DEPTH_LDS_MAX_THREADS && threads % 64 == 0 && threads <= keys / 2,
            "threads of m = %lld", (long long)m);
  }
  REQUIRE(erpl_depth_lds_keys(L) == L && (size_t)erpl_depth_lds_keys(L) * 8 <= 160 * 1024, "the limit fits the LDS of a CU");
  REQUIRE(erpl_depth_group_rows(17, 21) == 21 && erpl_depth_group_rows(2147483647LL, 4096) == 1, "rows of a group");
  REQUIRE((size_t)erpl_depth_group_rows(1048576, 4096) * 1048576 * 16 <= ERPL_DEPTH_KEY_BYTES, "a group fits its bytes");
  printf("ok path\n");
  return true;
}

bool check_layout() {
  const int64_t ms[] = {1, 2, 255, 256, 257, 16384, 16385, 65536, 65537, 1048576, 2147483647LL};
  for (int64_t m : ms)
    for (int C : {1, 8})
      for (int T : {1, 4096})
        for (int32_t limit : {0, 16})
          for (size_t temp : {(size_t)0, (size_t)12345}) {
            const ErplDepthLayout l = erpl_depth_layout(m, C, T, limit, temp);
            REQUIRE(l.lds == erpl_depth_use_lds(m, limit) && (l.lds ? l.group == 0 : (l.group >= 1 && l.group <= T)), "the path of m = %lld",
                    (long long)m);
            const size_t g = l.group > 1 ? (size_t)l.group : 1;
            REQUIRE(l.lds || m > ERPL_DEPTH_SEG_MAX || g * (size_t)m < ((size_t)1 << 32), "the offsets of a group are 32-bit");
            const size_t at[] = {l.pair, l.rown, l.keys, l.offs, l.temp, l.chan, l.rows, l.count};
            const size_t size[] = {(size_t)T * (size_t)m * 8, (size_t)T * 4, 2 * g * (size_t)m * 8, (g + 1) * 4, temp, (size_t)C * 64,
                                   (size_t)C * (size_t)T * 64, 32};
            size_t end = 0;
            for (int k = 0; k < 8; ++k) {
              REQUIRE(at[k] % 256 == 0 && at[k] >= end, "piece %d of m = %lld", k, (long long)m);
              REQUIRE(at[k] + size[k] >= at[k], "piece %d of m = %lld overflows", k, (long long)m);
              end = at[k] + size[k];
            }
            REQUIRE(l.need >= end && l.need - end < 256, "need of m = %lld", (long long)m);
          }
  // the largest call: 4096 rows of 2^31 - 1 columns are 2^46 bytes of pairs, far inside 64 bits
  const ErplDepthLayout l = erpl_depth_layout(2147483647LL, 8, 4096, 0, 0);
  REQUIRE(l.need > ((size_t)1 << 46) && l.need < ((size_t)1 << 47), "need at the shape limits: %zu", l.need);
  static_assert(sizeof(erpl_depth_row) == 64 && sizeof(erpl_depth_spec) == 32, "the records of the C ABI");
  printf("ok layout\n");
  return true;
}

}  // namespace

int main() {
  if (!check_cov() || !check_h() || !check_fences() || !check_path() || !check_layout()) return 1;
  printf("ok erpl_depth_check\n");
  return 0;
}
