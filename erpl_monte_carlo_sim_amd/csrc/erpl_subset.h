// erpl_subset.h — the rule of subset simulation (erpl_mc_subset_* of include/erpl_mc.h), one definition for the host
// (erpl_mc_subset_*_host, erpl_subset_check.cpp) and the device (erpl_subset.hip).  Internal: never installed.  Every unit
// that includes it is built without FMA contraction.  Subset simulation: Au & Beck, Probabilistic Engineering Mechanics 16
// (2001); the proposal is the conditional sampling (pCN) step in standard-normal space of Papaioannou, Betz, Zwirglmaier &
// Straub, Probabilistic Engineering Mechanics 41 (2015).
//
// THE CONTRACT
// Layout   A level's population is a matrix [R][ld] of N = T C columns: C chains of T steps, STEP-MAJOR - the column of step t
//          of chain j is t C + j.  A round reads the contiguous block of C columns of step t - 1 and writes the block of step
//          t.  The level's [16][N] summaries, its status words, its g and its indicator bytes are laid out alike.
// g        the limit state of a sample (erpl_subset_g): without a centre g = sign * summary[row]; with (cx, cy)
//          dx = x - cx, dy = y - cy over the rows ERPL_SUM_IMPACT_X / _Y and g = sign * sqrt(dx * dx + dy * dy), one rounding
//          per operation.  g = -inf where erpl_why_of(..) != 0 (the filter of erpl_mc_analyze), where the status word carries
//          ERPL_ST_NAN or ERPL_ST_INCOMPLETE, or where the value is not finite.  A NaN g handed in by a caller counts as -inf
//          in everything below (erpl_subset_key).
// Order    a is before b iff g_a > g_b, or g_a == g_b and id_a < id_b: ascending in (~erpl_tally_key(g), id); -0.0 is below
//          +0.0.  The SEEDS of a level are the first C samples in this order, the threshold b is the g of the last of them,
//          selected[i] = 1 exactly for those C, and idx lists them ascending in id.  Fewer than C samples with g > -inf:
//          "the level has died out", ERPL_ERR_INVALID on the host; the device call writes n_alive and leaves the comparison
//          to its caller (it cannot refuse without waiting).
// Proposal for chain j (global), row r, level l, step t: Philox4x32-10, key (seed lo, seed hi), counter
//          (j >> 1, r | t << 16, l, 3) - tag 3 of counter word 3, see erpl_philox.h; even j takes o0 | o1 << 32, odd j
//          o2 | o3 << 32; u = ((draw >> 11) + 0.5) 2^-53, the one u that rounds up to 1 taken as 1 - 2^-53
//          (erpl_design_p, ERPL_DESIGN_RANDOM).
//          normal row   x' = rho_r x + s_r xi, xi = erpl_design_ppnd16(u), s_r = sqrt(1 - rho_r^2) from the caller: two
//                       products and one addition, each rounded once.
//          uniform row  v = x + w_r (u - 0.5); v < 0: v += 1; then v >= 1: v -= 1; a v that rounding left at <= 0 becomes the
//                       smallest positive double, one at >= 1 becomes 1 - 2^-53.  A symmetric proposal on the circle: the
//                       uniform law is kept without an acceptance ratio.
//          Limits: t <= 65535, R <= ERPL_DESIGN_MAX_ROWS, C < 2^31, l < 2^32.  Everything but xi is integer work plus
//          correctly rounded +, -, *: uniform rows are the same bits on the host and on the device.  xi goes through the
//          platform's log and sqrt: on either side |x' - (rho_r x + s_r Phi^-1(u))| <= s_r 8e-15 max(1, |xi|) +
//          2^-50 (|rho_r x| + |s_r xi|) - the bar of erpl_mc_design's normal rows against the exact quantile plus the three
//          roundings - so host and device differ by at most twice that.
// Commit   a candidate is accepted iff g_cand >= b (false for a NaN); the next column is the candidate's (primitives,
//          summary, status, g) if accepted and the current one otherwise.
// Chain statistics of an indicator I (a byte per column, counted as I != 0): n1 = sum I, and for k = 1 .. T - 1
//          pair[k - 1] = sum over chains j and steps t < T - k of I[t C + j] I[(t + k) C + j]; all int64.  The host makes of
//          them (erpl_subset_delta2), with p = n1 / N: R(k) = pair[k - 1] / (N - k C) - p^2,
//          gamma = 2 sum_k (1 - k / T) R(k) / (p (1 - p)), delta^2 = (1 - p) / (p N) (1 + gamma) (gamma = 0 at level 0);
//          P = prod p_l, c.o.v. = sqrt(sum delta_l^2): Au & Beck's estimate, which ignores the correlation between levels
//          and therefore runs low.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "erpl_design.h"
#include "erpl_mc.h"
#include "erpl_tally.h"

#define ERPL_SUBSET_HD ERPL_PHILOX_HD

// ---------------------------------------------------------------- the limit state

// g of one sample: v[] its 16 summary values, st its status word (has_status false: none)
ERPL_SUBSET_HD double erpl_subset_g(const erpl_subset_spec& s, const double* v, bool has_status, int32_t st) {
  const ErplFilter f = {s.max_apogee, s.min_apogee, s.max_range, s.max_flight_time, s.energy_apogee};
  if (erpl_why_of(f, v[ERPL_SUM_APOGEE_ALT], v[ERPL_SUM_RANGE], v[ERPL_SUM_FLIGHT_TIME]) != 0) return -(double)INFINITY;
  if (has_status && (st & (ERPL_ST_NAN | ERPL_ST_INCOMPLETE))) return -(double)INFINITY;
  double x;
  if (s.use_centre) {
    const double dx = v[ERPL_SUM_IMPACT_X] - s.cx, dy = v[ERPL_SUM_IMPACT_Y] - s.cy;
    const double xx = dx * dx, yy = dy * dy;
    x = sqrt(xx + yy);
  } else {
    x = v[s.row];
  }
  if (!erpl_is_finite(x)) return -(double)INFINITY;
  return s.sign < 0 ? -x : x;
}

// ---------------------------------------------------------------- the order

// ascending in this key = descending in g; NaN shares the key of -inf (the largest key any g has)
ERPL_SUBSET_HD uint64_t erpl_subset_key(double g) { return ~erpl_tally_key(g != g ? -(double)INFINITY : g); }
ERPL_SUBSET_HD double erpl_subset_g_of_key(uint64_t key) { return erpl_double_of(erpl_tally_bits_of_key(~key)); }
ERPL_SUBSET_HD bool erpl_subset_alive(double g) { return g > -(double)INFINITY; }   // false for a NaN

// ---------------------------------------------------------------- the proposal

// u of (chain j, row, level, step), strictly inside (0, 1)
ERPL_SUBSET_HD double erpl_subset_u(uint64_t seed, uint32_t level, uint32_t step, uint32_t row, uint32_t chain) {
  const ErplPhiloxOut o = erpl_philox4x32_10(chain >> 1, row | (step << 16), level, 3u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t draw = (chain & 1u) ? ((uint64_t)o.w[2] | ((uint64_t)o.w[3] << 32)) : ((uint64_t)o.w[0] | ((uint64_t)o.w[1] << 32));
  const double u = ((double)(draw >> 11) + 0.5) * 0x1p-53;
  return erpl_design_p(ERPL_DESIGN_RANDOM, 0u, u, 1u);
}

ERPL_SUBSET_HD double erpl_subset_step_normal(double x, double rho, double s, double u) {
  const double a = rho * x, b = s * erpl_design_ppnd16(u);
  return a + b;
}

ERPL_SUBSET_HD double erpl_subset_step_uniform(double x, double w, double u) {
  const double h = u - 0.5;
  double v = x + w * h;
  if (v < 0.0) v += 1.0;
  if (v >= 1.0) v -= 1.0;
  if (!(v > 0.0)) v = 0x1p-1074;
  if (v >= 1.0) v = erpl_design_below(1.0);
  return v;
}

ERPL_SUBSET_HD double erpl_subset_candidate(bool normal, double x, double rho, double s, double w, uint64_t seed, uint32_t level,
                                            uint32_t step, uint32_t row, uint32_t chain) {
  const double u = erpl_subset_u(seed, level, step, row, chain);
  return normal ? erpl_subset_step_normal(x, rho, s, u) : erpl_subset_step_uniform(x, w, u);
}

// ---------------------------------------------------------------- the host side: the rules behind the _host calls

// one (src, dst) pair of erpl_mc_subset_seeds, one (cand, cur, next) triple of erpl_mc_subset_commit: column `from` of a
// matrix into column `to` of another, row by row
inline void erpl_subset_copy_column(const void* src, int64_t ld_src, int64_t from, void* dst, int64_t ld_dst, int64_t to, int rows,
                                    int elem) {
  for (int r = 0; r < rows; ++r)
    memcpy((char*)dst + ((int64_t)r * ld_dst + to) * elem, (const char*)src + ((int64_t)r * ld_src + from) * elem, (size_t)elem);
}

// the arguments have been checked (erpl_subset.hip); false: the level has died out (nothing but *n_alive is written)
inline bool erpl_subset_seeds_rule(const double* g, int64_t n, int64_t n_seeds, int32_t* idx, uint8_t* selected, double* threshold,
                                   int64_t* n_alive, const erpl_subset_gather* gathers, int n_gathers) {
  int64_t alive = 0;
  for (int64_t i = 0; i < n; ++i) alive += erpl_subset_alive(g[i]) ? 1 : 0;
  if (n_seeds == 0) {   // the indicator of a given threshold
    int64_t count = 0;
    for (int64_t i = 0; i < n; ++i) { selected[i] = g[i] >= *threshold ? 1 : 0; count += selected[i]; }
    *n_alive = count;
    return true;
  }
  *n_alive = alive;
  if (alive < n_seeds) return false;
  std::vector<int32_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = (int32_t)i;
  auto before = [&](int32_t a, int32_t b) {
    const uint64_t ka = erpl_subset_key(g[a]), kb = erpl_subset_key(g[b]);
    return ka < kb || (ka == kb && a < b);
  };
  std::nth_element(order.begin(), order.begin() + (n_seeds - 1), order.end(), before);
  *threshold = erpl_subset_g_of_key(erpl_subset_key(g[order[(size_t)(n_seeds - 1)]]));
  std::sort(order.begin(), order.begin() + n_seeds);
  for (int64_t i = 0; i < n; ++i) selected[i] = 0;
  for (int64_t k = 0; k < n_seeds; ++k) {
    idx[k] = order[(size_t)k];
    selected[idx[k]] = 1;
    for (int q = 0; q < n_gathers; ++q)
      erpl_subset_copy_column(gathers[q].src, gathers[q].ld_src, idx[k], gathers[q].dst, gathers[q].ld_dst, k, gathers[q].rows,
                              gathers[q].elem_size);
  }
  return true;
}

inline void erpl_subset_propose_rule(const erpl_subset_spec& sp, const uint8_t* kinds, const double* rho, const double* s,
                                     const double* w, int rows, const double* cur, int64_t ld, int64_t first_chain, int64_t count,
                                     double* cand, int64_t ld_cand) {
  for (int r = 0; r < rows; ++r)
    for (int64_t c = 0; c < count; ++c)
      cand[(int64_t)r * ld_cand + c] = erpl_subset_candidate(kinds[r] == ERPL_DESIGN_NORMAL, cur[(int64_t)r * ld + c], rho[r], s[r], w[r],
                                                             sp.seed, sp.level, sp.step, (uint32_t)r, (uint32_t)(first_chain + c));
}

inline void erpl_subset_commit_rule(double threshold, const double* g_cand, const double* g_cur, double* g_next,
                                    const erpl_subset_triple* triples, int n_triples, int64_t count, int64_t* n_accepted) {
  int64_t acc = 0;
  for (int64_t c = 0; c < count; ++c) {
    const bool take = g_cand[c] >= threshold;
    acc += take ? 1 : 0;
    g_next[c] = take ? g_cand[c] : g_cur[c];
    for (int q = 0; q < n_triples; ++q) {
      const erpl_subset_triple& t = triples[q];
      if (take) erpl_subset_copy_column(t.cand, t.ld_cand, c, t.next, t.ld, c, t.rows, t.elem_size);
      else erpl_subset_copy_column(t.cur, t.ld, c, t.next, t.ld, c, t.rows, t.elem_size);
    }
  }
  *n_accepted += acc;
}

inline void erpl_subset_chain_stats_rule(const uint8_t* sel, int64_t C, int64_t T, int64_t* n1, int64_t* pair) {
  int64_t ones = 0;
  for (int64_t i = 0; i < C * T; ++i) ones += sel[i] ? 1 : 0;
  *n1 = ones;
  for (int64_t k = 1; k < T; ++k) {
    int64_t sum = 0;
    for (int64_t t = 0; t + k < T; ++t)
      for (int64_t j = 0; j < C; ++j) sum += (sel[t * C + j] && sel[(t + k) * C + j]) ? 1 : 0;
    pair[k - 1] = sum;
  }
}

// delta^2 of a level from its chain statistics (chained false: level 0, gamma = 0); *gamma_out receives gamma.  p = 0 or
// p = 1: NaN and 0.
inline double erpl_subset_delta2(int64_t n1, const int64_t* pair, int64_t C, int64_t T, bool chained, double* gamma_out) {
  const double N = (double)(C * T), p = (double)n1 / N;
  double gamma = 0.0;
  if (chained && n1 > 0 && n1 < C * T) {
    double sum = 0.0;
    for (int64_t k = 1; k < T; ++k) {
      const double Rk = (double)pair[k - 1] / (N - (double)(k * C)) - p * p;
      sum += (1.0 - (double)k / (double)T) * Rk;
    }
    gamma = 2.0 * sum / (p * (1.0 - p));
  }
  *gamma_out = gamma;
  return (1.0 - p) / (p * N) * (1.0 + gamma);
}
