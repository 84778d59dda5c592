// erpl_pce_check — erpl_pce.h on the host alone (no HIP, no library): what must hold before a kernel uses it.  Over a grid of
// shapes (n_vars, degree, order) the enumeration gives as many terms as the closed form, in the contract's order (total degree,
// then number of variables, then variable tuple, then degree tuple, each ascending), none twice, every one within the shape.
// The univariate bases are orthonormal under their laws: the Gram matrix of psi_0 .. psi_12 under a 40-point Gauss-Legendre
// rule on (0, 1) and under a 40-point Gauss-Hermite rule (nodes by Newton's iteration on the recurrences, here in long
// double) is the identity within 1e-11.  Prints one line per check; exit status 1 on the first violation.  Build with a host
// sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_pce.h"

namespace {
typedef long double ld;
const ld kPi = 3.141592653589793238462643383279502884L;

// nodes in (0, 1) and weights that sum to 1 of the N-point Gauss-Legendre rule
void gauss_legendre(int N, std::vector<double>& x, std::vector<double>& w) {
  x.resize(N); w.resize(N);
  for (int i = 0; i < N; ++i) {
    ld t = cosl(kPi * (i + 0.75L) / (N + 0.5L)), dp = 0;
    for (int it = 0; it < 100; ++it) {
      ld p0 = 1, p1 = t;
      for (int k = 1; k < N; ++k) { const ld p2 = ((2 * k + 1) * t * p1 - k * p0) / (k + 1); p0 = p1; p1 = p2; }
      dp = N * (t * p1 - p0) / (t * t - 1);
      const ld step = p1 / dp;
      t -= step;
      if (fabsl(step) < 1e-19L) break;
    }
    x[i] = (double)((t + 1) / 2);
    w[i] = (double)(1 / ((1 - t * t) * dp * dp));   // 2 / ((1 - t^2) P'^2), halved for the law on (0, 1)
  }
}

// nodes and weights (sum 1) of the N-point Gauss rule of the standard normal law: the roots of He_N
void gauss_hermite(int N, std::vector<double>& x, std::vector<double>& w) {
  x.resize(N); w.resize(N);
  std::vector<ld> root(N);
  // the roots interlace: bisection between the roots of He_{N-1}, from He_1's root 0 on
  std::vector<ld> prev(1, 0.0L);
  auto he = [](int n, ld t) { ld h0 = 1, h1 = t; if (n == 0) return h0; for (int k = 1; k < n; ++k) { const ld h2 = t * h1 - k * h0; h0 = h1; h1 = h2; } return h1; };
  for (int n = 2; n <= N; ++n) {
    std::vector<ld> cur(n);
    const ld edge = 2 * sqrtl((ld)n) + 2;
    for (int i = 0; i < n; ++i) {
      ld lo = i == 0 ? -edge : prev[i - 1], hi = i == n - 1 ? edge : prev[i];
      const bool up = he(n, lo) < 0;
      for (int it = 0; it < 200; ++it) {
        const ld mid = (lo + hi) / 2;
        if ((he(n, mid) < 0) == up) lo = mid; else hi = mid;
      }
      cur[i] = (lo + hi) / 2;
    }
    prev = cur;
  }
  ld fact = 1;
  for (int k = 2; k < N; ++k) fact *= k;   // (N - 1)!
  for (int i = 0; i < N; ++i) {
    const ld h = he(N - 1, prev[i]);
    x[i] = (double)prev[i];
    w[i] = (double)(fact / (N * h * h));
  }
}

bool orthonormal(const char* name, int kind, const std::vector<double>& x, const std::vector<double>& w) {
  ErplPceTables tab;
  erpl_pce_make_tables(&tab);
  const int D = ERPL_SUR_MAX_DEGREE;
  std::vector<ld> gram((size_t)(D + 1) * (D + 1), 0.0L);
  double u[ERPL_SUR_MAX_DEGREE];
  for (size_t q = 0; q < x.size(); ++q) {
    erpl_pce_univariate(tab, kind, x[q], D, u, 1);
    for (int a = 0; a <= D; ++a)
      for (int b = 0; b <= D; ++b) gram[(size_t)a * (D + 1) + b] += (ld)w[q] * (a ? u[a - 1] : 1.0) * (b ? u[b - 1] : 1.0);
  }
  ld worst = 0;
  for (int a = 0; a <= D; ++a)
    for (int b = 0; b <= D; ++b) {
      const ld err = fabsl(gram[(size_t)a * (D + 1) + b] - (a == b ? 1 : 0));
      if (err > worst) worst = err;
    }
  printf("%s %s: largest deviation of the Gram matrix from the identity %.3Le\n", worst <= 1e-11L ? "ok" : "FAIL", name, worst);
  return worst <= 1e-11L;
}

// -1, 0, 1: term a before, equal to, behind term b in the contract's order
int compare_terms(const int8_t* a, const int8_t* b) {
  int ga = 0, gb = 0, oa = 0, ob = 0;
  for (int s = 0; s < ERPL_PCE_SLOTS; ++s) {
    ga += a[2 * s + 1]; gb += b[2 * s + 1];
    oa += a[2 * s] >= 0; ob += b[2 * s] >= 0;
  }
  if (ga != gb) return ga < gb ? -1 : 1;
  if (oa != ob) return oa < ob ? -1 : 1;
  for (int s = 0; s < oa; ++s)
    if (a[2 * s] != b[2 * s]) return a[2 * s] < b[2 * s] ? -1 : 1;
  for (int s = 0; s < oa; ++s)
    if (a[2 * s + 1] != b[2 * s + 1]) return a[2 * s + 1] < b[2 * s + 1] ? -1 : 1;
  return 0;
}
}  // namespace

int main() {
  const int T = 2 * ERPL_PCE_SLOTS;
  long checked = 0;
  for (int V = 1; V <= ERPL_SUR_MAX_VARS; ++V)
    for (int p = 1; p <= ERPL_SUR_MAX_DEGREE; ++p)
      for (int o = 1; o <= ERPL_SUR_MAX_ORDER; ++o) {
        const int64_t P = erpl_pce_count(V, p, o);
        if (erpl_pce_enumerate(V, p, o, nullptr, 0) != P) {
          printf("FAIL n_vars=%d degree=%d order=%d: the enumeration does not give the closed form's %lld terms\n", V, p, o, (long long)P);
          return 1;
        }
        if (P > 4 * ERPL_SUR_MAX_TERMS) continue;   // counted; the order is checked on what fits four times the limit
        std::vector<int8_t> terms((size_t)P * T);
        erpl_pce_enumerate(V, p, o, terms.data(), P);
        for (int64_t t = 0; t < P; ++t) {
          const int8_t* tm = &terms[(size_t)t * T];
          int g = 0, used = 0;
          bool ok = true;
          for (int s = 0; s < ERPL_PCE_SLOTS; ++s) {
            if (tm[2 * s] >= 0) {
              ok = ok && used == s && tm[2 * s] < V && tm[2 * s + 1] >= 1 && (s == 0 || tm[2 * s] > tm[2 * s - 2]);
              ++used;
              g += tm[2 * s + 1];
            } else {
              ok = ok && tm[2 * s] == -1 && tm[2 * s + 1] == 0;
            }
          }
          ok = ok && g <= p && used <= o && (t > 0) == (used > 0);
          // strictly ascending in the contract's order: also no term twice
          if (ok && t > 0) ok = compare_terms(tm - T, tm) < 0;
          if (!ok) {
            printf("FAIL n_vars=%d degree=%d order=%d: term %lld is outside the shape or out of order\n", V, p, o, (long long)t);
            return 1;
          }
        }
        ++checked;
      }
  printf("ok terms: closed form == enumeration on %d shapes, order and uniqueness on %ld of them\n",
         ERPL_SUR_MAX_VARS * ERPL_SUR_MAX_DEGREE * ERPL_SUR_MAX_ORDER, checked);
  const struct { int V, p, o; long long want; } known[] = {{1, 1, 1, 2},   {1, 12, 1, 13},  {2, 12, 2, 91},  {3, 12, 3, 455},
                                                          {4, 8, 4, 495}, {6, 6, 4, 887},  {25, 3, 2, 976}, {32, 2, 2, 561},
                                                          {32, 12, 1, 385}, {11, 4, 3, 1035}, {3, 10, 3, 286}};
  for (const auto& k : known)
    if (erpl_pce_count(k.V, k.p, k.o) != k.want) {
      printf("FAIL n_vars=%d degree=%d order=%d: %lld terms, the contract says %lld\n", k.V, k.p, k.o,
             (long long)erpl_pce_count(k.V, k.p, k.o), k.want);
      return 1;
    }
  printf("ok counts: the known answers of the contract\n");
  std::vector<double> x, w;
  gauss_legendre(40, x, w);
  if (!orthonormal("legendre", ERPL_DESIGN_UNIFORM, x, w)) return 1;
  gauss_hermite(40, x, w);
  if (!orthonormal("hermite", ERPL_DESIGN_NORMAL, x, w)) return 1;
  return 0;
}
