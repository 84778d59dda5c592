// erpl_pce.h — the polynomial chaos basis of erpl_mc_surrogate, one definition for the host (erpl_mc_surrogate_terms,
// erpl_mc_surrogate_predict_host, erpl_pce_check.cpp) and the device (the kernels of erpl_surrogate.hip).  Internal: never
// installed.  The contract is in include/erpl_mc.h; in short:
//   tables      a_k = (2k+1)/(k+1), b_k = k/(k+1), s_k = sqrt(2k+1), h_k = 1/sqrt(k!), made on the host at call time
//   uniform     x = 2u - 1; P0 = 1, P1 = x, P_{k+1} = ((a_k x) P_k) - (b_k P_{k-1}); psi_k = s_k P_k
//   normal      He0 = 1, He1 = z, He_{k+1} = (z He_k) - ((double)k He_{k-1}); psi_k = h_k He_k
//   terms       multi-indices with |alpha|_1 <= degree and at most `order` variables, in ONE order: total degree, number of
//               variables, variable tuple (lexicographic), degree tuple (lexicographic); term 0 is the constant
//   a term      the product of its psi factors in ascending variable order, starting from the first factor
//   the value   acc = c_0, then acc = acc + (c_alpha Psi_alpha) in ascending term index
// Only *, - and + on doubles and table look-ups: the same bits on the host and on the device as long as the unit is built
// without FMA contraction.  The univariate values of one sample live in u[((v * degree) + (k - 1)) * stride] for variable v
// and degree k >= 1 (psi_0 = 1 is never stored): stride 1 on the host, the workgroup's sample count in LDS on the device.
#pragma once
#include <math.h>
#include <stdint.h>

#include "erpl_mc.h"

#if defined(__HIPCC__)
#define ERPL_PCE_HD __host__ __device__ inline
#else
#define ERPL_PCE_HD inline
#endif

#define ERPL_PCE_SLOTS ERPL_SUR_MAX_ORDER   // (variable, degree) pairs of a term

// the four tables, by degree 0 .. ERPL_SUR_MAX_DEGREE
struct ErplPceTables {
  double a[ERPL_SUR_MAX_DEGREE + 1], b[ERPL_SUR_MAX_DEGREE + 1], s[ERPL_SUR_MAX_DEGREE + 1], h[ERPL_SUR_MAX_DEGREE + 1];
};

// host only: every entry one correctly rounded operation on exact integers (12! < 2^53), sqrt included
inline void erpl_pce_make_tables(ErplPceTables* t) {
  double fact = 1.0;
  for (int k = 0; k <= ERPL_SUR_MAX_DEGREE; ++k) {
    if (k > 0) fact = fact * (double)k;
    t->a[k] = (double)(2 * k + 1) / (double)(k + 1);
    t->b[k] = (double)k / (double)(k + 1);
    t->s[k] = sqrt((double)(2 * k + 1));
    t->h[k] = 1.0 / sqrt(fact);
  }
}

ERPL_PCE_HD bool erpl_pce_finite(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// psi_1 .. psi_degree of one variable of one sample into u[0], u[stride], ..
ERPL_PCE_HD void erpl_pce_univariate(const ErplPceTables& t, int kind, double v, int degree, double* u, int stride) {
  if (kind == ERPL_DESIGN_NORMAL) {
    double prev = 1.0, cur = v;
    u[0] = t.h[1] * cur;
    for (int k = 1; k < degree; ++k) {
      const double next = (v * cur) - ((double)k * prev);
      prev = cur; cur = next;
      u[k * stride] = t.h[k + 1] * cur;
    }
  } else {
    const double x = 2.0 * v - 1.0;
    double prev = 1.0, cur = x;
    u[0] = t.s[1] * cur;
    for (int k = 1; k < degree; ++k) {
      const double next = ((t.a[k] * x) * cur) - (t.b[k] * prev);
      prev = cur; cur = next;
      u[k * stride] = t.s[k + 1] * cur;
    }
  }
}

// One term of one sample: term = its ERPL_PCE_SLOTS (variable, degree) pairs, unused slots (-1, 0) behind the used ones.
// The constant term (no used slot) is 1.
ERPL_PCE_HD double erpl_pce_term(const int8_t* term, const double* u, int degree, int stride) {
  if (term[0] < 0) return 1.0;
  double v = u[((int)term[0] * degree + ((int)term[1] - 1)) * stride];
  for (int s = 1; s < ERPL_PCE_SLOTS; ++s) {
    if (term[2 * s] < 0) break;
    v = v * u[((int)term[2 * s] * degree + ((int)term[2 * s + 1] - 1)) * stride];
  }
  return v;
}

// The fitted polynomial of one sample from its univariate values: coef[P], terms[P][ERPL_PCE_SLOTS][2].
ERPL_PCE_HD double erpl_pce_value(const double* coef, const int8_t* terms, int n_terms, const double* u, int degree, int stride) {
  double acc = coef[0];
  for (int t = 1; t < n_terms; ++t) acc = acc + (coef[t] * erpl_pce_term(terms + (size_t)t * 2 * ERPL_PCE_SLOTS, u, degree, stride));
  return acc;
}

// C(n, k) for n <= 32: exact in 64 bits, every intermediate quotient is an integer
ERPL_PCE_HD int64_t erpl_pce_choose(int n, int k) {
  if (k < 0 || k > n) return 0;
  int64_t c = 1;
  for (int i = 1; i <= k; ++i) c = c * (int64_t)(n - k + i) / (int64_t)i;
  return c;
}

// P = 1 + sum_{g=1..degree} sum_{o=1..min(order, g, n_vars)} C(n_vars, o) C(g - 1, o - 1)
ERPL_PCE_HD int64_t erpl_pce_count(int n_vars, int degree, int order) {
  int64_t p = 1;
  for (int g = 1; g <= degree; ++g)
    for (int o = 1; o <= order && o <= g && o <= n_vars; ++o) p += erpl_pce_choose(n_vars, o) * erpl_pce_choose(g - 1, o - 1);
  return p;
}

// Host only: the terms in the contract's order into terms[cap][ERPL_PCE_SLOTS][2] (NULL: counted only).  Returns the number
// of terms the shape has; nothing is written from term `cap` on.
inline int64_t erpl_pce_enumerate(int n_vars, int degree, int order, int8_t* terms, int64_t cap) {
  int64_t n = 0;
  auto emit = [&](int o, const int* var, const int* deg) {
    if (terms && n < cap) {
      int8_t* t = terms + n * 2 * ERPL_PCE_SLOTS;
      for (int s = 0; s < ERPL_PCE_SLOTS; ++s) {
        t[2 * s] = (int8_t)(s < o ? var[s] : -1);
        t[2 * s + 1] = (int8_t)(s < o ? deg[s] : 0);
      }
    }
    ++n;
  };
  int var[ERPL_PCE_SLOTS] = {0, 0, 0, 0}, deg[ERPL_PCE_SLOTS] = {0, 0, 0, 0};
  emit(0, var, deg);
  for (int g = 1; g <= degree; ++g)
    for (int o = 1; o <= order && o <= g && o <= n_vars; ++o) {
      for (int s = 0; s < o; ++s) var[s] = s;
      for (;;) {   // variable tuples, lexicographic
        // degree tuples: compositions of g into o parts >= 1, lexicographic; the last part is what the others leave
        for (int s = 0; s < o - 1; ++s) deg[s] = 1;
        deg[o - 1] = g - (o - 1);
        for (;;) {
          emit(o, var, deg);
          // the rightmost part that can grow: the parts behind it (their sum is `tail`) keep at least 1 each
          int s = o - 2, tail = deg[o - 1];
          while (s >= 0 && tail - 1 < o - 1 - s) { tail += deg[s]; --s; }
          if (s < 0) break;
          deg[s] += 1;
          tail -= 1;
          for (int r = s + 1; r < o - 1; ++r) { deg[r] = 1; tail -= 1; }
          deg[o - 1] = tail;
        }
        int s = o - 1;   // the next variable tuple
        while (s >= 0 && var[s] == n_vars - o + s) --s;
        if (s < 0) break;
        ++var[s];
        for (int r = s + 1; r < o; ++r) var[r] = var[r - 1] + 1;
      }
    }
  return n;
}
