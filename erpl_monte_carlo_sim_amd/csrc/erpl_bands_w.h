// erpl_bands_w.h — the rule of erpl_mc_corridor_bands_weighted (include/erpl_mc.h): every (channel, node) row of a time-resolved
// matrix described under the integer weights erpl_mc_reweight wrote.  One definition for the host
// (erpl_mc_corridor_bands_weighted_host, erpl_bands_w_check.cpp) and for what the host makes of the device's sums
// (erpl_corridor_w.hip).  Internal: never installed.  Every unit that includes it is built without FMA contraction.
//
// THE CONTRACT
// Weights  admitted iff 0 <= W_i <= 2^Q, Q = erpl_rw_q(m), for EVERY column of the call, masked or not (erpl_bw_scan).  max_w is
//          the largest over all m columns, K its bit length (0 for an all-zero row), w_i = W_i 2^-K: exact, in [0, 1).
// Rows     the population of a row is its own: mask byte 0, the value finite, W_i > 0.  A column with mask byte 0 that is not in
//          it is NON_FINITE (the value is not finite) or, failing that, ZERO (W_i == 0).
// Exact    count, n_non_finite, n_zero, sum_w = sum W, exceed[j] = sum W [x > thr_j] (integer adds: they commute); quantile q =
//          the value at 0-based rank T - 1 of the multiset in which column i occurs W_i times, T = erpl_rw_target(q, sum_w)
//          (erpl_reweight.h), in the order of erpl_tally_key; min and max in that order too (the sign of a zero extreme is exact).
// Doubles  S_d = sum_w 2^-K; sum_wx = sum w x, sum_w2 = sum w w, a2[j] = sum w w [x > thr_j]; mean = sum_wx / S_d; with
//          d = x - mean, dd = d d: m2 = sum w dd, se2 = sum (w w) dd.  The host adds the terms in index order with a compensated
//          sum (ErplRwSum); the device adds per thread in index order and folds in the fixed order of erpl_stat_device.h.  What
//          is made of the sums exists once: erpl_bw_finish.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "erpl_mc.h"
#include "erpl_reweight.h"
#include "erpl_tally.h"

// what the passes over one row hand back: 208 bytes
struct ErplBwRaw {
  uint64_t count, n_non_finite, n_zero, sum_w;
  uint64_t exceed[ERPL_BANDS_W_MAX_THRESHOLDS];
  uint64_t key[ERPL_RW_MAX_Q];                   // erpl_tally_key of the selected order statistics
  double vmin, vmax, sum_wx, mean, m2, se2, sum_w2;
  double a2[ERPL_BANDS_W_MAX_THRESHOLDS];
};

// what the first pass over the weight row hands back
struct ErplBwScan {
  uint64_t n_masked;
  uint64_t max_w;                                // over the admitted weights of all m columns
  int64_t first_bad;                             // the lowest column whose weight is outside 0 .. 2^Q, or -1
};

// K of a call: the bit length of max_w
ERPL_RW_HD int erpl_bw_bits(uint64_t max_w) {
  int k = 0;
  while (k < 64 && (max_w >> k) != 0ull) ++k;
  return k;
}

// Host only: the first pass
inline ErplBwScan erpl_bw_scan(const int64_t* weights, const uint8_t* mask, int64_t m) {
  ErplBwScan s = {0ull, 0ull, -1};
  const int64_t most = (int64_t)1 << erpl_rw_q(m);
  for (int64_t i = 0; i < m; ++i) {
    const int64_t W = weights[i];
    if (mask && mask[i]) ++s.n_masked;
    if (W < 0 || W > most) { if (s.first_bad < 0) s.first_bad = i; continue; }
    if ((uint64_t)W > s.max_w) s.max_w = (uint64_t)W;
  }
  return s;
}

// Host only: the record of a row from its sums.  An empty row (count == 0): the integers 0, every double NaN.
inline void erpl_bw_finish(const erpl_bands_w_spec& sp, int channel, const ErplBwRaw& r, int K, erpl_bands_w_row* o) {
  memset(o, 0, sizeof(*o));
  o->count = (int64_t)r.count; o->n_non_finite = (int64_t)r.n_non_finite; o->n_zero = (int64_t)r.n_zero;
  const bool empty = r.count == 0 || r.sum_w == 0;
  const double nan = NAN;
  o->min = o->max = o->mean = o->var = o->std = o->mean_se = o->sum_w2 = o->ess = nan;
  for (int k = 0; k < ERPL_RW_MAX_Q; ++k) o->quantile[k] = nan;
  for (int k = 0; k < ERPL_BANDS_W_MAX_THRESHOLDS; ++k) o->a2[k] = nan;
  if (empty) return;
  const double S = ldexp((double)r.sum_w, -K);
  o->sum_w = (int64_t)r.sum_w;
  o->min = r.vmin; o->max = r.vmax;
  o->mean = r.mean;
  o->var = r.m2 / S;
  o->std = sqrt(o->var);
  o->mean_se = sqrt(r.se2) / S;
  o->sum_w2 = r.sum_w2;
  o->ess = S * S / r.sum_w2;
  for (int k = 0; k < sp.n_q; ++k) o->quantile[k] = erpl_double_of(erpl_tally_bits_of_key(r.key[k]));
  for (int k = 0; k < sp.n_thresholds[channel]; ++k) {
    o->exceed_w[k] = (int64_t)r.exceed[k];
    o->a2[k] = r.a2[k];
  }
}

// Host only: the sums of one row, x[0 .. m - 1], in index order
inline void erpl_bw_row_host(const erpl_bands_w_spec& sp, int channel, const double* x, const uint8_t* mask, const int64_t* weights,
                             int64_t m, int K, ErplBwRaw* out) {
  ErplBwRaw r = {};
  uint64_t kmin = ~0ull, kmax = 0ull;            // the extremes go by key: -0.0 below +0.0
  const int n_thr = sp.n_thresholds[channel];
  const double* thr = sp.threshold[channel];
  std::vector<int64_t> w((size_t)m, 0);          // the weight of a member, 0 outside the population
  ErplRwSum sum_wx, sum_w2, m2, se2, a2[ERPL_BANDS_W_MAX_THRESHOLDS];
  for (int64_t i = 0; i < m; ++i) {
    if (mask && mask[i]) continue;
    const double v = x[i];
    if (!erpl_is_finite(v)) { ++r.n_non_finite; continue; }
    const int64_t W = weights[i];
    if (W == 0) { ++r.n_zero; continue; }
    w[(size_t)i] = W;
    const double wd = ldexp((double)W, -K);
    ++r.count;
    r.sum_w += (uint64_t)W;
    sum_wx.add(wd * v);
    sum_w2.add(wd * wd);
    kmin = erpl_tally_key(v) < kmin ? erpl_tally_key(v) : kmin;
    kmax = erpl_tally_key(v) > kmax ? erpl_tally_key(v) : kmax;
    for (int k = 0; k < n_thr; ++k)
      if (v > thr[k]) { r.exceed[k] += (uint64_t)W; a2[k].add(wd * wd); }
  }
  r.vmin = r.count ? erpl_double_of(erpl_tally_bits_of_key(kmin)) : (double)INFINITY;
  r.vmax = r.count ? erpl_double_of(erpl_tally_bits_of_key(kmax)) : -(double)INFINITY;
  r.sum_wx = sum_wx.value(); r.sum_w2 = sum_w2.value();
  for (int k = 0; k < n_thr; ++k) r.a2[k] = a2[k].value();
  r.mean = r.sum_wx / ldexp((double)r.sum_w, -K);
  for (int64_t i = 0; i < m; ++i) {
    if (w[(size_t)i] == 0) continue;
    const double wd = ldexp((double)w[(size_t)i], -K), d = x[i] - r.mean;
    const double dd = d * d;
    m2.add(wd * dd);
    se2.add((wd * wd) * dd);
  }
  r.m2 = m2.value(); r.se2 = se2.value();
  if (r.sum_w > 0 && sp.n_q > 0) {
    uint64_t T[ERPL_RW_MAX_Q];
    for (int k = 0; k < sp.n_q; ++k) T[k] = erpl_rw_target(sp.q[k], r.sum_w);
    erpl_rw_select_host(x, w.data(), m, T, sp.n_q, r.key);
  }
  *out = r;
}

// Host only: the whole call behind the refusals.  Returns the lowest column with a weight that is not admitted (nothing has been
// written then), or -1.
inline int64_t erpl_bw_host(const erpl_bands_w_spec& sp, const double* values, const uint8_t* mask, const int64_t* weights, int64_t m,
                            int64_t ld, erpl_bands_w_row* rows, erpl_bands_w_result* result) {
  const ErplBwScan scan = erpl_bw_scan(weights, mask, m);
  if (scan.first_bad >= 0) return scan.first_bad;
  const int K = erpl_bw_bits(scan.max_w);
  for (int c = 0; c < sp.n_channels; ++c)
    for (int k = 0; k < sp.n_nodes; ++k) {
      const int64_t r = (int64_t)c * sp.n_nodes + k;
      ErplBwRaw raw;
      erpl_bw_row_host(sp, c, values + r * ld, mask, weights, m, K, &raw);
      erpl_bw_finish(sp, c, raw, K, &rows[r]);
    }
  memset(result, 0, sizeof(*result));
  result->m = m; result->n_masked = (int64_t)scan.n_masked; result->n_counted = m - (int64_t)scan.n_masked;
  result->max_w = (int64_t)scan.max_w; result->K = K; result->Q = erpl_rw_q(m);
  return -1;
}

// The refusals of both calls, in the order of the header; `fail` formats the text and returns the code.
typedef int (*ErplBwFail)(int code, const char* fmt, ...);
inline int erpl_bw_check(const erpl_bands_w_spec* s, const double* values, const int64_t* weights, const erpl_bands_w_row* rows,
                         const erpl_bands_w_result* result, int64_t m, int64_t ld, ErplBwFail fail) {
  if (!s) return fail(ERPL_ERR_INVALID, "spec is NULL");
  if (s->n_channels < 1 || s->n_channels > ERPL_CORRIDOR_MAX_CHANNELS)
    return fail(ERPL_ERR_INVALID, "spec->n_channels = %d outside 1..%d", s->n_channels, ERPL_CORRIDOR_MAX_CHANNELS);
  if (s->n_nodes < 1 || s->n_nodes > ERPL_CORRIDOR_MAX_NODES)
    return fail(ERPL_ERR_INVALID, "spec->n_nodes = %d outside 1..%d", s->n_nodes, ERPL_CORRIDOR_MAX_NODES);
  if (s->n_q < 0 || s->n_q > ERPL_RW_MAX_Q) return fail(ERPL_ERR_INVALID, "spec->n_q = %d outside 0..%d", s->n_q, ERPL_RW_MAX_Q);
  for (int k = 0; k < s->n_q; ++k)
    if (!(s->q[k] >= 0.0 && s->q[k] <= 1.0)) return fail(ERPL_ERR_INVALID, "spec->q[%d] = %g outside [0, 1]", k, s->q[k]);
  for (int c = 0; c < s->n_channels; ++c)
    if (s->n_thresholds[c] < 0 || s->n_thresholds[c] > ERPL_BANDS_W_MAX_THRESHOLDS)
      return fail(ERPL_ERR_INVALID, "spec->n_thresholds[%d] = %d outside 0..%d", c, s->n_thresholds[c], ERPL_BANDS_W_MAX_THRESHOLDS);
  for (int c = 0; c < s->n_channels; ++c)
    for (int k = 0; k < s->n_thresholds[c]; ++k)
      if (s->threshold[c][k] != s->threshold[c][k]) return fail(ERPL_ERR_INVALID, "spec->threshold[%d][%d] is NaN", c, k);
  if (!values) return fail(ERPL_ERR_INVALID, "values is NULL");
  if (!weights) return fail(ERPL_ERR_INVALID, "weights is NULL");
  if (!rows) return fail(ERPL_ERR_INVALID, "rows is NULL");
  if (!result) return fail(ERPL_ERR_INVALID, "result is NULL");
  if (m <= 0 || m > 2147483647LL) return fail(ERPL_ERR_INVALID, "m = %lld outside 1..2^31 - 1", (long long)m);
  if (ld < m) return fail(ERPL_ERR_INVALID, "ld = %lld is below m = %lld", (long long)ld, (long long)m);
  return ERPL_OK;
}
