// erpl_reweight.h — the rule of erpl_mc_reweight (include/erpl_mc.h): the statistics of a flown run under another input law, by
// importance weights.  One definition for the host (erpl_mc_reweight_host, erpl_reweight_check.cpp) and the device
// (erpl_reweight.hip).  Internal: never installed.  Every unit that includes it is built without FMA contraction: every
// operation named below rounds once, on its own.
//
// THE CONTRACT
// Law      n_law rows (1 .. ERPL_RW_MAX_LAW) of independent primitives, each flown under N(0, 1) (ERPL_DESIGN_NORMAL) or U(0, 1)
//          (ERPL_DESIGN_UNIFORM).  The target of a normal row is N(mu, s^2): t = (z - mu) / s, l_r = c_r + 0.5 * (z * z - t * t),
//          c_r = -log(s).  The target of a uniform row is U(a, b), 0 <= a < b <= 1: l_r = c_r = -log(b - a) where a <= u <= b and
//          -inf elsewhere.  c_r is computed ONCE, ON THE HOST, with libm's log (erpl_rw_law_of) and handed to the kernel as a
//          constant: what a column then needs is +, -, *, /, so the host and the device give the same bits.
//          The log-weight of column i is l_i = (((0.0 + l_0) + l_1) + ..) in the order of the law rows.
// exp      erpl_rw_exp(x), x <= 0, neither libm nor OCML: 0 below -64 (and for a NaN); k = rint(x * log2 e);
//          r = (x - k * ln2_hi) - k * ln2_lo (fdlibm's split); s = the Horner form of sum_{j <= 13} r^j / j!; ldexp(s, k).
//          Within 1 ulp of libm's exp on [-64, 0], exp(0) == 1 exactly, no value above 1.
// Weights  Q = min(52, 62 - ceil(log2 n)) from the call's n; W_i = (int64) floor(ldexp(erpl_rw_exp(l_i - l_max), Q)) with l_max
//          the maximum over the population, 0 outside it.  The heaviest column has W = 2^Q exactly, every W is exact in a
//          double, and S = sum W <= n 2^Q <= 2^62.
// Columns  in this order: MASKED (mask byte != 0), NON_FINITE (a law row or a requested outcome row is not finite), OUTSIDE
//          (l_i is not above -inf: outside the support of a uniform target), otherwise in the POPULATION.
// Order statistics  quantile q is the value at 0-based rank T - 1 of the multiset in which column i occurs W_i times,
//          T = clamp((uint64) ceil(q * (double) S), 1, S): np.quantile(x, q, weights = W, method = "inverted_cdf").  The order
//          is the library's key (erpl_tally_key: -0.0 just below +0.0); the value returned is a value of the row.
// Doubles  sum_w2 = sum W^2 (w * w rounded, then added); per row sum W x, then with mean = sum W x / S and d = x - mean:
//          m2 = sum W (d * d), se2 = sum (W * W) (d * d); per threshold A2 = sum W^2 [x > thr].  The host adds the terms in
//          index order with a compensated sum (ErplRwSum); the device adds per thread in index order and folds in the fixed
//          order of erpl_stat_device.h: the two agree to rounding, each repeats itself bit for bit.  What is made of the sums
//          exists once: erpl_rw_result.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "erpl_mc.h"
#include "erpl_tally.h"

#define ERPL_RW_HD ERPL_TALLY_HD

enum { ERPL_RW_IN = 0, ERPL_RW_MASKED = 1, ERPL_RW_NON_FINITE = 2, ERPL_RW_OUTSIDE = 3 };

// the law as the kernels take it (by value): the spec's rows and their constants c_r
struct ErplRwLaw {
  int32_t n_law;
  uint8_t normal[ERPL_RW_MAX_LAW];
  double mu[ERPL_RW_MAX_LAW], s[ERPL_RW_MAX_LAW], a[ERPL_RW_MAX_LAW], b[ERPL_RW_MAX_LAW], c[ERPL_RW_MAX_LAW];
};

// Host only: c_r through libm's log
inline ErplRwLaw erpl_rw_law_of(const erpl_rw_spec& sp) {
  ErplRwLaw law = {};
  law.n_law = sp.n_law;
  for (int r = 0; r < sp.n_law; ++r) {
    law.normal[r] = sp.kind[r] == ERPL_DESIGN_NORMAL;
    law.mu[r] = sp.mu[r]; law.s[r] = sp.s[r]; law.a[r] = sp.a[r]; law.b[r] = sp.b[r];
    law.c[r] = law.normal[r] ? -log(sp.s[r]) : -log(sp.b[r] - sp.a[r]);
  }
  return law;
}

// l_r of one value of law row r
ERPL_RW_HD double erpl_rw_row(const ErplRwLaw& law, int r, double x) {
  if (law.normal[r]) {
    const double t = (x - law.mu[r]) / law.s[r];
    const double zz = x * x, tt = t * t;
    const double d = zz - tt;
    const double h = 0.5 * d;
    return law.c[r] + h;
  }
  return (law.a[r] <= x && x <= law.b[r]) ? law.c[r] : -(double)INFINITY;
}

// exp(x) for x <= 0
ERPL_RW_HD double erpl_rw_exp(double x) {
  if (!(x >= -64.0)) return 0.0;
  const double k = rint(x * 1.4426950408889634);
  const double hi = k * 6.93147180369123816490e-01, lo = k * 1.90821492927058770002e-10;
  const double r = (x - hi) - lo;
  double s = 1.6059043836821613e-10;             // 1 / 13!
  s = s * r + 2.08767569878681e-09;              // 1 / 12!
  s = s * r + 2.505210838544172e-08;
  s = s * r + 2.755731922398589e-07;
  s = s * r + 2.7557319223985893e-06;
  s = s * r + 2.48015873015873e-05;
  s = s * r + 0.0001984126984126984;
  s = s * r + 0.001388888888888889;
  s = s * r + 0.008333333333333333;
  s = s * r + 0.041666666666666664;
  s = s * r + 0.16666666666666666;
  s = s * r + 0.5;
  s = s * r + 1.0;
  s = s * r + 1.0;
  return ldexp(s, (int)k);
}

// Q of a call over n >= 1 columns: n 2^Q <= 2^62
ERPL_RW_HD int erpl_rw_q(int64_t n) {
  int bits = 0;                                  // ceil(log2 n)
  while (bits < 62 && ((int64_t)1 << bits) < n) ++bits;
  const int q = 62 - bits;
  return q < 52 ? q : 52;
}

// W of a column of the population
ERPL_RW_HD int64_t erpl_rw_weight(double l, double lmax, int Q) { return (int64_t)floor(ldexp(erpl_rw_exp(l - lmax), Q)); }

// T of quantile q among S > 0 units of weight: the order statistic wanted is the one at 0-based rank T - 1
ERPL_RW_HD uint64_t erpl_rw_target(double q, uint64_t S) {
  const double t = ceil(q * (double)S);
  if (!(t >= 1.0)) return 1ull;
  if (t >= 18446744073709551616.0) return S;
  const uint64_t T = (uint64_t)t;
  return T > S ? S : T;
}

// where outcome row `row` of a column lives: a summary row or the caller's `extra`
ERPL_RW_HD double erpl_rw_outcome(const double* summary, int64_t ld_s, const double* extra, int row, int64_t i) {
  return row == ERPL_RW_ROW_EXTRA ? extra[i] : summary[(int64_t)row * ld_s + i];
}

// The state of column i and, in the population or outside the support, its log-weight.
ERPL_RW_HD int erpl_rw_column(const ErplRwLaw& law, const int32_t* rows, int n_rows, const double* factors, int64_t ld,
                              const double* summary, int64_t ld_s, const double* extra, const uint8_t* mask, int64_t i, double* l_out) {
  *l_out = NAN;
  if (mask && mask[i]) return ERPL_RW_MASKED;
  bool finite = true;
  double l = 0.0;
  for (int r = 0; r < law.n_law; ++r) {
    const double x = factors[(int64_t)r * ld + i];
    finite = finite && erpl_is_finite(x);
    l = l + erpl_rw_row(law, r, x);
  }
  for (int j = 0; j < n_rows; ++j) finite = finite && erpl_is_finite(erpl_rw_outcome(summary, ld_s, extra, rows[j], i));
  if (!finite) return ERPL_RW_NON_FINITE;
  if (!(l > -(double)INFINITY)) { *l_out = -(double)INFINITY; return ERPL_RW_OUTSIDE; }
  *l_out = l;
  return ERPL_RW_IN;
}

// ---------------------------------------------------------------- what the passes hand back, and what is made of it

struct ErplRwRawRow {
  double sum_wx, mean, vmin, vmax, m2, se2;
  uint64_t key[ERPL_RW_MAX_Q];                   // erpl_tally_key of the selected order statistics
  uint64_t exceed[ERPL_RW_MAX_THRESHOLDS];
  double a2[ERPL_RW_MAX_THRESHOLDS];
};
struct ErplRwRaw {
  uint64_t n_masked, n_non_finite, n_outside, count, n_zero, sum_w;
  double lmax, max_w, sum_w2;
  ErplRwRawRow row[ERPL_RW_MAX_ROWS];
};

// Host only: E[w_r^2] in closed form, multiplied over the rows; the share is 0 where the variance of the weights is infinite
inline double erpl_rw_expected_share(const erpl_rw_spec& sp) {
  double prod = 1.0;
  for (int r = 0; r < sp.n_law; ++r) {
    if (sp.kind[r] == ERPL_DESIGN_NORMAL) {
      const double s = sp.s[r], mu = sp.mu[r], v = 2.0 - s * s;
      if (!(v > 0.0)) return 0.0;
      prod *= exp(mu * mu / v) / (s * sqrt(v));
    } else {
      prod *= 1.0 / (sp.b[r] - sp.a[r]);
    }
  }
  return 1.0 / prod;
}

// Host only: the result of a call over n columns from its sums.  An empty population (count == 0 or S == 0): the integers of
// the weights (sum_w, max_w, exceed_w) 0 and every double that depends on the data NaN; the counts stay what they are.
inline void erpl_rw_result(const erpl_rw_spec& sp, const ErplRwRaw& raw, int64_t n, erpl_reweight* out) {
  *out = erpl_reweight{};
  out->n = n;
  out->n_masked = (int64_t)raw.n_masked; out->n_non_finite = (int64_t)raw.n_non_finite; out->n_outside = (int64_t)raw.n_outside;
  out->count = (int64_t)raw.count;
  out->Q = erpl_rw_q(n);
  out->n_zero = (int64_t)raw.n_zero;
  out->ess_expected_share = erpl_rw_expected_share(sp);
  const bool empty = raw.count == 0 || raw.sum_w == 0;
  const double S = (double)raw.sum_w;
  out->sum_w2 = out->ess = NAN;
  if (!empty) {
    out->sum_w = (int64_t)raw.sum_w;
    out->max_w = (int64_t)raw.max_w;
    out->sum_w2 = raw.sum_w2;
    out->ess = S * S / raw.sum_w2;
  }
  for (int j = 0; j < ERPL_RW_MAX_ROWS; ++j) {
    erpl_rw_row_stats& o = out->row[j];
    o.mean = o.mean_se = o.var = o.std = o.min = o.max = NAN;
    for (int k = 0; k < ERPL_RW_MAX_Q; ++k) o.quantile[k] = NAN;
    for (int k = 0; k < ERPL_RW_MAX_THRESHOLDS; ++k) o.p[k] = o.p_se[k] = NAN;
    if (empty || j >= sp.n_rows) continue;
    const ErplRwRawRow& r = raw.row[j];
    o.mean = r.mean;
    o.var = r.m2 / S;
    o.std = sqrt(o.var);
    o.mean_se = sqrt(r.se2) / S;
    o.min = r.vmin; o.max = r.vmax;
    for (int k = 0; k < sp.n_q; ++k) o.quantile[k] = erpl_double_of(erpl_tally_bits_of_key(r.key[k]));
    for (int k = 0; k < sp.n_thresholds[j]; ++k) {
      o.exceed_w[k] = (int64_t)r.exceed[k];
      const double p = (double)r.exceed[k] / S;
      const double a = (1.0 - 2.0 * p) * r.a2[k], b = (p * p) * raw.sum_w2;
      const double v = a + b;                    // (1 - p)^2 A2 + p^2 (sum_w2 - A2) >= 0; rounding may leave it just below
      o.p[k] = p;
      o.p_se[k] = sqrt(v > 0.0 ? v : 0.0) / S;
    }
  }
}

// ---------------------------------------------------------------- the rule on the host

// Host only: a compensated sum (Neumaier) in index order - the yardstick of the device's folded sums, so it loses nothing to
// the length of the run
struct ErplRwSum {
  double s = 0.0, c = 0.0;
  void add(double v) {
    const double t = s + v;
    c += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
    s = t;
  }
  double value() const { return s + c; }
};

// Host only: key[k] = the key at 0-based rank T[k] - 1 of the multiset in which x[i] occurs w[i] times (T[k] in 1 .. sum w):
// one stable sort serves every target
inline void erpl_rw_select_host(const double* x, const int64_t* w, int64_t n, const uint64_t* T, int n_targets, uint64_t* key) {
  std::vector<int64_t> order;
  for (int64_t i = 0; i < n; ++i)
    if (w[i] > 0) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](int64_t p, int64_t q) { return erpl_tally_key(x[p]) < erpl_tally_key(x[q]); });
  for (int k = 0; k < n_targets; ++k) {
    uint64_t cum = 0;
    key[k] = 0ull;
    for (int64_t i : order) {
      cum += (uint64_t)w[i];
      if (cum >= T[k]) { key[k] = erpl_tally_key(x[i]); break; }
    }
  }
}

// Host only: the whole call.  logw / weights may be NULL.
inline void erpl_rw_host(const erpl_rw_spec& sp, const double* factors, int64_t ld, const double* summary, int64_t ld_s, const double* extra,
                         const uint8_t* mask, int64_t n, erpl_reweight* result, double* logw, int64_t* weights) {
  const ErplRwLaw law = erpl_rw_law_of(sp);
  const int Q = erpl_rw_q(n);
  ErplRwRaw raw = {};
  std::vector<double> l((size_t)n);
  std::vector<int64_t> w((size_t)n, 0);
  raw.lmax = -(double)INFINITY;
  for (int64_t i = 0; i < n; ++i) {
    const int state = erpl_rw_column(law, sp.rows, sp.n_rows, factors, ld, summary, ld_s, extra, mask, i, &l[(size_t)i]);
    raw.n_masked += state == ERPL_RW_MASKED; raw.n_non_finite += state == ERPL_RW_NON_FINITE; raw.n_outside += state == ERPL_RW_OUTSIDE;
    if (state == ERPL_RW_IN) {
      ++raw.count;
      raw.lmax = l[(size_t)i] > raw.lmax ? l[(size_t)i] : raw.lmax;
    }
    if (logw) logw[i] = l[(size_t)i];
  }
  raw.max_w = -(double)INFINITY;
  ErplRwSum sum_w2;
  for (int64_t i = 0; i < n; ++i) {
    if (l[(size_t)i] > -(double)INFINITY) {
      const int64_t wi = erpl_rw_weight(l[(size_t)i], raw.lmax, Q);
      const double wd = (double)wi;
      w[(size_t)i] = wi;
      raw.sum_w += (uint64_t)wi;
      sum_w2.add(wd * wd);
      raw.n_zero += wi == 0;
      raw.max_w = wd > raw.max_w ? wd : raw.max_w;
    }
    if (weights) weights[i] = w[(size_t)i];
  }
  raw.sum_w2 = sum_w2.value();
  if (raw.count == 0) raw.max_w = 0.0;
  const double S = (double)raw.sum_w;
  std::vector<double> x((size_t)n);
  for (int j = 0; j < sp.n_rows; ++j) {
    ErplRwRawRow& r = raw.row[j];
    r.vmin = (double)INFINITY; r.vmax = -(double)INFINITY;
    ErplRwSum sum_wx, m2, se2, a2[ERPL_RW_MAX_THRESHOLDS];
    for (int64_t i = 0; i < n; ++i) {
      const int64_t wi = w[(size_t)i];
      if (wi == 0) { x[(size_t)i] = 0.0; continue; }
      const double v = erpl_rw_outcome(summary, ld_s, extra, sp.rows[j], i), wd = (double)wi;
      x[(size_t)i] = v;
      sum_wx.add(wd * v);
      r.vmin = v < r.vmin ? v : r.vmin;
      r.vmax = v > r.vmax ? v : r.vmax;
      for (int k = 0; k < sp.n_thresholds[j]; ++k)
        if (v > sp.threshold[j][k]) { r.exceed[k] += (uint64_t)wi; a2[k].add(wd * wd); }
    }
    r.sum_wx = sum_wx.value();
    for (int k = 0; k < sp.n_thresholds[j]; ++k) r.a2[k] = a2[k].value();
    r.mean = r.sum_wx / S;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t wi = w[(size_t)i];
      if (wi == 0) continue;
      const double wd = (double)wi, d = x[(size_t)i] - r.mean;
      const double dd = d * d;
      m2.add(wd * dd);
      se2.add((wd * wd) * dd);
    }
    r.m2 = m2.value(); r.se2 = se2.value();
    if (raw.sum_w > 0) {
      uint64_t T[ERPL_RW_MAX_Q];
      for (int k = 0; k < sp.n_q; ++k) T[k] = erpl_rw_target(sp.q[k], raw.sum_w);
      erpl_rw_select_host(x.data(), w.data(), n, T, sp.n_q, r.key);
    }
  }
  erpl_rw_result(sp, raw, n, result);
}
