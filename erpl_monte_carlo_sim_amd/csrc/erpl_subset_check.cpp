// erpl_subset_check — erpl_subset.h on the host alone (no HIP, no library): what must hold before a kernel runs anywhere.
//   1. a window of proposals (first_chain, count) equals those columns of the whole, bit for bit; uniform rows stay in (0, 1)
//   2. a whole subset run on a linear limit state in 24 dimensions (22 normal rows of weight 1 / sqrt(22), 2 uniform rows g
//      ignores), through the rules of the _host calls, gives the same bytes twice and a probability within a factor of e^2
//      of the exact Phi(-3.0902) = 1e-3
//   3. the seed selection: ties across the threshold admitted lowest id first, -inf, NaN, -0.0 below +0.0, n_seeds = 1 and
//      n_seeds = n, the died-out level
//   4. the chain statistics against a count that walks chain by chain
// Prints one ok line per part; exit status 1 on the first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_subset.h"

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

constexpr int kRows = 24, kNormal = 22;

void row_parameters(std::vector<uint8_t>& kinds, std::vector<double>& rho, std::vector<double>& s, std::vector<double>& w) {
  kinds.assign(kRows, ERPL_DESIGN_NORMAL);
  kinds[kRows - 2] = kinds[kRows - 1] = ERPL_DESIGN_UNIFORM;
  rho.assign(kRows, 0.8);
  s.assign(kRows, sqrt(1.0 - 0.8 * 0.8));
  w.assign(kRows, sqrt(1.0 - 0.8 * 0.8));
}

bool check_windows() {
  std::vector<uint8_t> kinds;
  std::vector<double> rho, s, w;
  row_parameters(kinds, rho, s, w);
  const int64_t C = 301, first = 37, count = 129, ld = C + 3;
  std::vector<double> cur((size_t)(kRows * ld)), whole((size_t)(kRows * ld), -7.0), win((size_t)(kRows * count), -7.0);
  for (int r = 0; r < kRows; ++r)
    for (int64_t c = 0; c < C; ++c) {
      const double u = erpl_design_jitter(11, (uint32_t)r, (uint64_t)c);
      cur[(size_t)(r * ld + c)] = kinds[r] == ERPL_DESIGN_NORMAL ? erpl_design_ppnd16(u) : u;
    }
  const uint32_t steps[3] = {1u, 7u, 65535u}, levels[2] = {0u, 0xffffffffu};
  for (uint32_t step : steps)
    for (uint32_t level : levels) {
      erpl_subset_spec sp = {};
      sp.seed = 0x123456789abcdefull; sp.level = level; sp.step = step;
      erpl_subset_propose_rule(sp, kinds.data(), rho.data(), s.data(), w.data(), kRows, cur.data(), ld, 0, C, whole.data(), ld);
      erpl_subset_propose_rule(sp, kinds.data(), rho.data(), s.data(), w.data(), kRows, cur.data() + first, ld, first, count, win.data(),
                               count);
      for (int r = 0; r < kRows; ++r) {
        REQUIRE(memcmp(&win[(size_t)(r * count)], &whole[(size_t)(r * ld + first)], (size_t)count * sizeof(double)) == 0,
                "step %u level %u row %d: the window differs from the whole", step, level, r);
        for (int64_t c = 0; c < C; ++c) {
          const double v = whole[(size_t)(r * ld + c)];
          REQUIRE(isfinite(v) && (kinds[r] == ERPL_DESIGN_NORMAL || (v > 0.0 && v < 1.0)), "row %d column %lld: %a", r, (long long)c, v);
        }
        REQUIRE(whole[(size_t)(r * ld + C)] == -7.0, "row %d: a store past count", r);
      }
    }
  // the wrap of a uniform row at both ends, and the clamps
  REQUIRE(erpl_subset_step_uniform(0.01, 1.0, 0.25) == 0.01 - 0.25 + 1.0, "wrap below 0");
  REQUIRE(erpl_subset_step_uniform(0.99, 1.0, 0.75) == (0.99 + 0.25) - 1.0, "wrap above 1");
  REQUIRE(erpl_subset_step_uniform(0.5, 1.0, 0.0) == 0x1p-1074, "v = 0 moves inside");
  REQUIRE(erpl_subset_step_uniform(0x1p-60, 0.0, 0.5) == 0x1p-60, "w = 0 is a copy");
  REQUIRE(erpl_subset_step_normal(1.25, 1.0, 0.0, 0.3) == 1.25 && erpl_subset_step_normal(1.25, 0.0, 1.0, 0.3) == erpl_design_ppnd16(0.3),
          "rho = 1 is a copy and rho = 0 a fresh draw");
  printf("ok windows\n");
  return true;
}

// g of the linear limit state: sum of the normal rows / sqrt(22), in row order
void linear_g(const double* x, int64_t ld, int64_t count, double* g) {
  const double wgt = 1.0 / sqrt((double)kNormal);
  for (int64_t c = 0; c < count; ++c) {
    double sum = 0.0;
    for (int r = 0; r < kNormal; ++r) sum += x[(int64_t)r * ld + c];
    g[c] = sum * wgt;
  }
}

struct Run {
  double probability, cov;
  int levels;
  int64_t evaluations;
  std::vector<double> population, thresholds;
};

bool subset_run(uint64_t seed, int64_t C, int64_t T, double target, Run* out) {
  std::vector<uint8_t> kinds;
  std::vector<double> rho, s, w;
  row_parameters(kinds, rho, s, w);
  const int64_t N = C * T;
  std::vector<double> pop((size_t)(kRows * N)), next((size_t)(kRows * N)), g((size_t)N), g_next((size_t)N), cand((size_t)(kRows * C)), g_cand((size_t)C);
  std::vector<int32_t> idx((size_t)C);
  std::vector<uint8_t> sel((size_t)N);
  std::vector<int64_t> pair((size_t)T);
  for (int r = 0; r < kRows; ++r)
    for (int64_t c = 0; c < N; ++c) {
      const double u = erpl_design_p(ERPL_DESIGN_RANDOM, 0u, erpl_design_jitter(seed, (uint32_t)r, (uint64_t)c), 1u);
      pop[(size_t)(r * N + c)] = kinds[r] == ERPL_DESIGN_NORMAL ? erpl_design_ppnd16(u) : u;
    }
  linear_g(pop.data(), N, N, g.data());
  out->evaluations = N;
  out->thresholds.clear();
  double P = 1.0, d2 = 0.0;
  for (int level = 0; level < 12; ++level) {
    double b = 0.0, gamma;
    int64_t alive = 0, n1 = 0;
    const erpl_subset_gather ga[2] = {{pop.data(), next.data(), N, N, kRows, 8}, {g.data(), g_next.data(), N, N, 1, 8}};
    REQUIRE(erpl_subset_seeds_rule(g.data(), N, C, idx.data(), sel.data(), &b, &alive, ga, 2), "level %d died out", level);
    if (b >= target) {   // the last level: the share beyond the target
      b = target;
      erpl_subset_seeds_rule(g.data(), N, 0, nullptr, sel.data(), &b, &alive, nullptr, 0);
      erpl_subset_chain_stats_rule(sel.data(), C, T, &n1, pair.data());
      P *= (double)n1 / (double)N;
      d2 += erpl_subset_delta2(n1, pair.data(), C, T, level > 0, &gamma);
      out->probability = P; out->cov = sqrt(d2); out->levels = level + 1; out->population = pop;
      return true;
    }
    out->thresholds.push_back(b);
    erpl_subset_chain_stats_rule(sel.data(), C, T, &n1, pair.data());
    REQUIRE(n1 == C, "level %d: %lld selected, %lld seeds", level, (long long)n1, (long long)C);
    P *= (double)n1 / (double)N;
    d2 += erpl_subset_delta2(n1, pair.data(), C, T, level > 0, &gamma);
    for (int64_t t = 1; t < T; ++t) {
      erpl_subset_spec sp = {};
      sp.seed = seed; sp.level = (uint32_t)(level + 1); sp.step = (uint32_t)t;
      const double* cur = next.data() + (t - 1) * C;
      erpl_subset_propose_rule(sp, kinds.data(), rho.data(), s.data(), w.data(), kRows, cur, N, 0, C, cand.data(), C);
      linear_g(cand.data(), C, C, g_cand.data());
      out->evaluations += C;
      const erpl_subset_triple tr = {cand.data(), cur, next.data() + t * C, C, N, kRows, 8};
      int64_t accepted = 0;
      erpl_subset_commit_rule(b, g_cand.data(), g_next.data() + (t - 1) * C, g_next.data() + t * C, &tr, 1, C, &accepted);
      REQUIRE(accepted >= 0 && accepted <= C, "accepted = %lld", (long long)accepted);
    }
    pop.swap(next);
    g.swap(g_next);
    for (int64_t c = 0; c < N; ++c) REQUIRE(g[(size_t)c] >= b, "level %d column %lld: g below the threshold", level, (long long)c);
  }
  REQUIRE(false, "the target was not reached in 12 levels");
}

bool check_run() {
  Run a, b;
  if (!subset_run(5, 512, 8, 3.0902, &a) || !subset_run(5, 512, 8, 3.0902, &b)) return false;
  REQUIRE(a.probability == b.probability && a.cov == b.cov && a.levels == b.levels && a.evaluations == b.evaluations &&
              memcmp(a.population.data(), b.population.data(), a.population.size() * sizeof(double)) == 0,
          "two runs of one seed differ");
  REQUIRE(fabs(log(a.probability / 1.0001e-3)) < 2.0, "P = %g against 1e-3", a.probability);
  REQUIRE(a.evaluations == 4096 + (int64_t)(a.levels - 1) * 3584, "%lld evaluations in %d levels", (long long)a.evaluations, a.levels);
  for (size_t l = 1; l < a.thresholds.size(); ++l) REQUIRE(a.thresholds[l] > a.thresholds[l - 1], "thresholds do not increase");
  printf("ok run P=%.6g cov=%.4f levels=%d evaluations=%lld\n", a.probability, a.cov, a.levels, (long long)a.evaluations);
  return true;
}

bool check_seeds() {
  const double inf = (double)INFINITY;
  //                  0    1    2     3    4    5     6    7    8     9
  const double g[] = {2.0, 5.0, -inf, 2.0, NAN, -0.0, 0.0, 2.0, 5.0, -inf};
  const int64_t n = 10;
  int32_t idx[10];
  uint8_t sel[10];
  double b;
  int64_t alive;
  // the order: 1, 8 (5.0), 0, 3, 7 (2.0), 6 (+0), 5 (-0), then 2, 4, 9 (-inf and NaN, by id)
  const int32_t order[10] = {1, 8, 0, 3, 7, 6, 5, 2, 4, 9};
  for (int64_t k = 1; k <= n; ++k) {
    const bool ok = erpl_subset_seeds_rule(g, n, k, idx, sel, &b, &alive, nullptr, 0);
    REQUIRE(alive == 7, "n_alive = %lld", (long long)alive);
    REQUIRE(ok == (k <= 7), "n_seeds = %lld: died out = %d", (long long)k, !ok);
    if (!ok) continue;
    std::vector<int32_t> want(order, order + k);
    std::sort(want.begin(), want.end());
    REQUIRE(memcmp(want.data(), idx, (size_t)k * sizeof(int32_t)) == 0, "n_seeds = %lld: idx", (long long)k);
    for (int64_t i = 0; i < n; ++i)
      REQUIRE(sel[i] == (std::find(want.begin(), want.end(), (int32_t)i) != want.end() ? 1 : 0), "n_seeds = %lld: selected[%lld]",
              (long long)k, (long long)i);
    const double last = g[order[k - 1]];
    REQUIRE(memcmp(&b, &last, sizeof b) == 0, "n_seeds = %lld: threshold %a", (long long)k, b);
  }
  // all equal, n_seeds = n; a gather of an int32 row
  const double same[5] = {1.5, 1.5, 1.5, 1.5, 1.5};
  const int32_t st[5] = {10, 11, 12, 13, 14};
  int32_t st_out[5] = {0, 0, 0, 0, 0};
  const erpl_subset_gather ga = {st, st_out, 5, 5, 1, 4};
  REQUIRE(erpl_subset_seeds_rule(same, 5, 3, idx, sel, &b, &alive, &ga, 1) && idx[0] == 0 && idx[1] == 1 && idx[2] == 2 && b == 1.5 &&
              st_out[0] == 10 && st_out[2] == 12 && st_out[3] == 0,
          "all equal: the first three by id");
  REQUIRE(erpl_subset_seeds_rule(same, 5, 5, idx, sel, &b, &alive, nullptr, 0) && idx[4] == 4 && sel[4] == 1, "n_seeds = n");
  // the indicator of a given threshold
  b = 2.0;
  REQUIRE(erpl_subset_seeds_rule(g, n, 0, nullptr, sel, &b, &alive, nullptr, 0) && alive == 5 && sel[0] && sel[1] && !sel[2] && !sel[4] && !sel[6],
          "the indicator of a threshold");
  printf("ok seeds\n");
  return true;
}

bool check_chain_stats() {
  const int64_t shapes[4][2] = {{130, 5}, {1, 2}, {7, 1}, {64, 9}};
  for (const auto& sh : shapes) {
    const int64_t C = sh[0], T = sh[1];
    for (int fill = 0; fill < 4; ++fill) {   // pseudo-random, all ones, all zeros, one chain all ones
      std::vector<uint8_t> sel((size_t)(C * T));
      for (int64_t i = 0; i < C * T; ++i)
        sel[(size_t)i] = fill == 0 ? (uint8_t)(erpl_fmix32((uint32_t)i + 17u) % 3u == 0u) : fill == 1 ? 1 : fill == 2 ? 0 : (uint8_t)(i % C == C / 2);
      std::vector<int64_t> pair((size_t)T, -1), want((size_t)T, 0);
      int64_t n1 = -1, ones = 0;
      erpl_subset_chain_stats_rule(sel.data(), C, T, &n1, pair.data());
      for (int64_t j = 0; j < C; ++j)
        for (int64_t t = 0; t < T; ++t) {
          if (!sel[(size_t)(t * C + j)]) continue;
          ones += 1;
          for (int64_t u = t + 1; u < T; ++u) want[(size_t)(u - t - 1)] += sel[(size_t)(u * C + j)];
        }
      REQUIRE(n1 == ones, "C = %lld T = %lld fill %d: n1", (long long)C, (long long)T, fill);
      for (int64_t k = 1; k < T; ++k)
        REQUIRE(pair[(size_t)(k - 1)] == want[(size_t)(k - 1)], "C = %lld T = %lld fill %d: pair[%lld]", (long long)C, (long long)T, fill, (long long)k);
      REQUIRE(pair[(size_t)(T - 1)] == -1, "a store past pair[T - 2]");
    }
  }
  printf("ok chain statistics\n");
  return true;
}
}  // namespace

int main() {
  if (!check_windows() || !check_seeds() || !check_chain_stats() || !check_run()) return 1;
  printf("ok erpl_subset_check\n");
  return 0;
}
