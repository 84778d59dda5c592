// erpl_debris_check — erpl_debris.h on the host alone (no HIP, no library): what must hold before a kernel runs anywhere.
//   1. directions: |d| within 4 ulp of 1 for 4096 ids of several (node, fragment) pairs; the uniforms never reach -1, 0 or 1;
//      the counter word keeps try, node and fragment apart
//   2. a window of ids gives the directions of those ids of the whole, bit for bit
//   3. the step rule at, one double below and one double above every threshold k0 * dt * 2^-m = stiff_limit, m = 0 .. 16, and
//      for 0, +inf and NaN
//   4. the ticks of a fall that is never halved give (n + wq) * dt to the bit; a halved step adds 2^(16 - m)
//   5. the fallback direction after sixteen rejections, through a source of pairs that never lands in the disc
// Prints one ok line per part; exit status 1 on the first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_debris.h"

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

const double kUlp = 0x1p-52;   // the spacing of doubles in [1, 2)

bool check_directions() {
  REQUIRE(erpl_debris_uniform(0ull) == -1.0 + 0x1p-52 && erpl_debris_uniform(~0ull) == 1.0 - 0x1p-52, "the ends of the uniform");
  REQUIRE(erpl_debris_uniform(1ull << 63) == 0x1p-52 && erpl_debris_uniform((1ull << 63) - 1) == -0x1p-52, "the uniform about 0");
  double worst = 0.0, mean[3] = {0.0, 0.0, 0.0};
  int most = 0;
  const int n = 4096;
  const uint32_t where[4][2] = {{0, 0}, {5, 3}, {4095, 63}, {64, 1}};
  for (int w = 0; w < 4; ++w)
    for (int i = 0; i < n; ++i) {
      ErplDebrisPhilox p;
      p.seed = 0x123456789abcdef0ull; p.id = (uint64_t)i + ((w == 2) ? (1ull << 33) : 0ull); p.node = where[w][0]; p.fragment = where[w][1];
      double d[3], e[3];
      const int tries = erpl_debris_direction_from(p, d);
      erpl_debris_direction(p.seed, p.id, p.node, p.fragment, e);
      REQUIRE(memcmp(d, e, sizeof(d)) == 0, "the two entry points differ at id %d", i);
      most = tries > most ? tries : most;
      const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      const double err = fabs(len - 1.0) / kUlp;
      worst = err > worst ? err : worst;
      REQUIRE(err <= 4.0, "|d| - 1 = %.3g ulp at id %d of (%u, %u)", err, i, p.node, p.fragment);
      if (w == 0) for (int c = 0; c < 3; ++c) mean[c] += d[c] / n;
    }
  for (int c = 0; c < 3; ++c) REQUIRE(fabs(mean[c]) <= 4.0 / sqrt(3.0 * n), "mean of component %d = %.4f", c, mean[c]);
  REQUIRE(most < ERPL_DEBRIS_MAX_TRIES, "a direction needed all %d tries", most);
  // try, node and fragment each change the draw; node 1 / fragment 0 is not node 0 / fragment 64
  ErplDebrisPhilox p = {7, 11, 3, 2}, q = p;
  double a0, b0, a1, b1;
  p(0, &a0, &b0);
  q.node = 4; q(0, &a1, &b1);
  REQUIRE(a0 != a1 || b0 != b1, "the node does not enter the draw");
  q = p; q.fragment = 3; q(0, &a1, &b1);
  REQUIRE(a0 != a1 || b0 != b1, "the fragment does not enter the draw");
  p(1, &a1, &b1);
  REQUIRE(a0 != a1 || b0 != b1, "the try does not enter the draw");
  printf("ok directions: |d| - 1 at most %.2f ulp, at most %d tries, means %.4f %.4f %.4f\n", worst, most, mean[0], mean[1], mean[2]);
  return true;
}

bool check_windows() {
  const int n = 701, first = 37, count = 129;
  std::vector<double> whole(3 * n), win(3 * count);
  for (int i = 0; i < n; ++i) erpl_debris_direction(99, (uint64_t)(1000 + 3 * i), 17, 5, &whole[3 * i]);
  for (int i = 0; i < count; ++i) erpl_debris_direction(99, (uint64_t)(1000 + 3 * (first + i)), 17, 5, &win[3 * i]);
  REQUIRE(memcmp(win.data(), &whole[3 * first], 3 * count * sizeof(double)) == 0, "the window's directions differ from the whole's");
  double other[3];
  erpl_debris_direction(100, 1000, 17, 5, other);
  REQUIRE(memcmp(other, whole.data(), sizeof(other)) != 0, "the seed does not enter the draw");
  printf("ok windows\n");
  return true;
}

bool check_step_rule() {
  const double dts[3] = {0.25, 0.05, 0.1}, limits[3] = {0.25, 1.0, 0.3};
  for (int c = 0; c < 3; ++c) {
    const double dt = dts[c], limit = limits[c];
    for (int m = 0; m <= ERPL_DEBRIS_TICK_BITS; ++m) {
      const double h = ldexp(dt, -m);
      // the largest k0 with k0 * h <= limit, found from the quotient by stepping one double at a time
      double k = limit / h;
      while (k * h > limit) k = nextafter(k, 0.0);
      while (nextafter(k, INFINITY) * h <= limit) k = nextafter(k, INFINITY);
      double sc;
      int got = erpl_debris_halvings(k, dt, limit, &sc);
      REQUIRE(got == m && sc == ldexp(1.0, -m), "at the threshold of m = %d (dt %g, limit %g): m = %d, scale %g", m, dt, limit, got, sc);
      if (m > 0) {
        got = erpl_debris_halvings(nextafter(k, 0.0), dt, limit, &sc);
        REQUIRE(got == m, "just below the threshold of m = %d: m = %d", m, got);
      }
      got = erpl_debris_halvings(nextafter(k, INFINITY), dt, limit, &sc);
      const int want = m < ERPL_DEBRIS_TICK_BITS ? m + 1 : ERPL_DEBRIS_TICK_BITS;
      REQUIRE(got == want && sc == ldexp(1.0, -want), "just above the threshold of m = %d: m = %d", m, got);
    }
    double sc;
    REQUIRE(erpl_debris_halvings(0.0, dt, limit, &sc) == 0 && sc == 1.0, "k0 = 0");
    REQUIRE(erpl_debris_halvings(INFINITY, dt, limit, &sc) == ERPL_DEBRIS_TICK_BITS && sc == 0x1p-16, "k0 = inf");
    REQUIRE(erpl_debris_halvings(NAN, dt, limit, &sc) == ERPL_DEBRIS_TICK_BITS && sc == 0x1p-16, "k0 = NaN");
  }
  printf("ok step rule\n");
  return true;
}

bool check_ticks() {
  const double dts[4] = {0.25, 0.05, 0.1, 1.0 / 3.0}, wqs[5] = {0.0, 1.0, 0.5, 0.3, 0.9999999999999999};
  for (double dt : dts)
    for (double wq : wqs) {
      int64_t ticks = 0;
      for (int n = 0; n <= 20000; ++n) {
        if (n % 37 == 0 || n == 20000) {
          const double got = erpl_debris_tfall(ticks, wq, 0, dt), want = ((double)n + wq) * dt;
          REQUIRE(got == want, "n = %d, wq = %.17g, dt = %.17g: %.17g, want %.17g", n, wq, dt, got, want);
        }
        ticks += erpl_debris_step_ticks(0);
      }
    }
  REQUIRE(erpl_debris_step_ticks(0) == 65536 && erpl_debris_step_ticks(7) == 512 && erpl_debris_step_ticks(16) == 1, "ticks of a step");
  // 3 whole steps, 2 half steps, then a crossing half way through a quarter step: 4.125 dt
  const int64_t ticks = 3 * erpl_debris_step_ticks(0) + 2 * erpl_debris_step_ticks(1);
  REQUIRE(erpl_debris_tfall(ticks, 0.5, 2, 0.25) == 4.125 * 0.25, "mixed steps: %.17g", erpl_debris_tfall(ticks, 0.5, 2, 0.25));
  // the largest count a call can reach, 2^20 steps, is exact in a double
  REQUIRE(erpl_debris_tfall((int64_t)(1 << 20) * 65536, 0.0, 0, 0.05) == 1048576.0 * 0.05, "2^20 steps");
  printf("ok ticks\n");
  return true;
}

// the test hook: a source of pairs outside the unit disc, which counts how often it is asked
struct NeverAccepted {
  mutable int asked = 0;
  mutable uint32_t last = 0;
  void operator()(uint32_t t, double* a, double* b) const {
    ++asked; last = t;
    *a = 0.9; *b = -0.9;
  }
};
struct ThirdAccepted {
  void operator()(uint32_t t, double* a, double* b) const {
    *a = t == 2 ? 0.5 : 0.9; *b = t == 2 ? -0.25 : 0.9;
  }
};

bool check_fallback() {
  NeverAccepted never;
  double d[3] = {7.0, 7.0, 7.0};
  const int tries = erpl_debris_direction_from(never, d);
  REQUIRE(tries == ERPL_DEBRIS_MAX_TRIES && never.asked == 16 && never.last == 15, "%d tries, asked %d times", tries, never.asked);
  REQUIRE(d[0] == 0.0 && d[1] == 0.0 && d[2] == 1.0, "the fallback is (%g, %g, %g)", d[0], d[1], d[2]);
  const int third = erpl_debris_direction_from(ThirdAccepted(), d);
  const double s = 0.5 * 0.5 + 0.25 * 0.25, q = sqrt(1.0 - s);
  REQUIRE(third == 3 && d[0] == 1.0 * q && d[1] == -0.5 * q && d[2] == 1.0 - 2.0 * s, "the third try: (%g, %g, %g)", d[0], d[1], d[2]);
  printf("ok fallback\n");
  return true;
}
}  // namespace

int main() {
  if (!(check_directions() && check_windows() && check_step_rule() && check_ticks() && check_fallback())) return 1;
  printf("ok erpl_debris_check\n");
  return 0;
}
