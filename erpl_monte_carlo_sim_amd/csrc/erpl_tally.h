// erpl_tally.h — what a sample contributes to a tally (erpl_mc_tally_* of include/erpl_mc.h), one definition for the host
// (erpl_mc_tally_*_host, erpl_tally_check.cpp) and the device (erpl_tally.hip).  Internal: never installed.  It also holds
// the three per-sample rules the resident statistics share with the tally, so that each exists once: the reason bits of
// erpl_mc_analyze (erpl_why_of), the bin rule and the edges of erpl_mc_histogram / _histogram_xy (erpl_bin_of, ErplEdges)
// and the crossing rule of erpl_mc_impact_density (erpl_zone_flips).  Every unit that includes it is built without FMA
// contraction; the one FMA of the rule is written out.
//
// THE CONTRACT
// Filter   why = erpl_why_of(bounds, apogee, range, flight_time); a sample is VALID iff why == 0.  Header words: n, n_valid,
//          one count per reason bit, one per termination code (status & 0xFF in 0..4), ERPL_ST_NAN, ERPL_ST_INCOMPLETE words
//          (status == NULL: those seven stay as they are).
// Rows     row j reads summary row rows[j].  A value x is COUNTED iff the sample is valid and x is finite.  Then
//            count += 1;  x < lo: below += 1;  x > hi: above += 1;  otherwise hist[erpl_bin_of(x, ..)] += 1
//            exceed[t] += 1 iff x > threshold[j][t]
//            d = x - centre[j] (one rounding).  !(|d| < 2^500): moment_skipped += 1 and nothing else; otherwise d goes into
//            the accumulator `sum_d`, and hi = d * d (one rounding), lo = |d| < 2^-485 ? 0 : fma(d, d, -hi) go into `sum_d2`.
//            With |d| in [2^-485, 2^500) hi + lo is d^2 exactly, and all three are multiples of 2^-1074 below 2^1000.
//          Extremes: the k smallest and the k largest counted values with their ids (first_id + column).  The order is the
//          key of the bit pattern (erpl_tally_key: -0 < +0), ties go to the lower id: `smallest` ascending by (key, id),
//          `largest` ascending by (~key, id).  Fewer than k counted values: fewer held.
// Grid     the pair (row_x, row_y): counted iff valid and both finite; inside iff lo <= v <= hi on both axes, then cell
//          erpl_bin_of(x) * bins_y + erpl_bin_of(y) += 1, otherwise outside += 1; zone_inside[z] += 1 iff the even-odd rule
//          of erpl_zone_flips over the polygon's edges puts the counted sample inside.
//
// THE STATE: int64 words, all zero when empty; offsets from erpl_tally_layout (the one place they are computed):
//   [0, 16)                n, n_valid, reason[6], termination[5], n_status_nan, n_incomplete, 0
//   per row j, in order    count, below, above, moment_skipped, exceed[8]               12 words  (row[j])
//                          hist[bins[j]]                                                          (hist[j])
//                          sum_d, sum_d2: two long accumulators                   2 x 70 words  (acc[j], acc[j] + 70)
//                          n_smallest, n_largest, smallest[k] x (bits, id), largest[k] x (bits, id)   (ext[j])
//   grid                   counted, outside, zone_inside[8]                            10 words  (grid)
//                          cells[bins_x * bins_y], x-major                                        (cells)
// A long accumulator is 70 digits of 32 bits, least significant first, one per int64 word: its value is
// sum_i w[i] 2^(32 i - 1088).  CANONICAL FORM: 0 <= w[i] < 2^32 for i < 69 and w[69] carries the sign (0 or -1 for every sum
// of fewer than 2^62 terms below 2^1000): two's complement in base 2^32, so one value has one representation.  A double
// m 2^e (|m| < 2^53, e >= -1074) lands on the three digits (e + 1088) / 32 + {0, 1, 2}, each part below 2^32 in magnitude:
// a word takes 2^31 parts before it could overflow, which is why the device may add the parts of a whole window with integer
// atomics and propagate the carries once.  After every add and every merge every accumulator is canonical, and held extremes
// are sorted with the unused entries zero: equal tallies are equal bytes, whatever the split, the order or the device.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "erpl_mc.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ERPL_TALLY_HD __host__ __device__ __forceinline__
#else
#define ERPL_TALLY_HD inline
#endif

#define ERPL_TALLY_HEADER_WORDS 16
#define ERPL_TALLY_ROW_WORDS 12    // count, below, above, moment_skipped, exceed[8]
#define ERPL_TALLY_GRID_WORDS 10   // counted, outside, zone_inside[8]
#define ERPL_TALLY_ACC_WORDS 70
#define ERPL_TALLY_ACC_BIAS 1088   // digit i weighs 2^(32 i - 1088)

// ---------------------------------------------------------------- the rules the resident statistics share with the tally

ERPL_TALLY_HD uint64_t erpl_bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}
ERPL_TALLY_HD double erpl_double_of(uint64_t b) {
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}
ERPL_TALLY_HD bool erpl_is_finite(double v) { return (erpl_bits_of(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// the order-preserving key of a finite double, -0.0 just below +0.0 (key_of_signed of erpl_stat_device.h), and its inverse
ERPL_TALLY_HD uint64_t erpl_tally_key(double v) {
  const uint64_t b = erpl_bits_of(v);
  return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
ERPL_TALLY_HD uint64_t erpl_tally_bits_of_key(uint64_t k) { return k ^ ((k >> 63) ? (1ull << 63) : ~0ull); }

// The reason bits of a sample (erpl_mc_analyze; monte_carlo.py:356-388 of the reference).  Comparisons with NaN are false.
struct ErplFilter {
  double max_apogee, min_apogee, max_range, max_flight_time, energy_apogee;
};
ERPL_TALLY_HD int erpl_why_of(const ErplFilter& f, double apo, double rng, double ft) {
  int why = 0;
  if (!erpl_is_finite(apo) || !erpl_is_finite(rng) || !erpl_is_finite(ft)) why |= ERPL_WHY_NON_FINITE;
  if (apo > f.max_apogee) why |= ERPL_WHY_APOGEE_HIGH;
  else if (apo < f.min_apogee) why |= ERPL_WHY_APOGEE_LOW;
  if (rng > f.max_range) why |= ERPL_WHY_RANGE;
  if (ft > f.max_flight_time) why |= ERPL_WHY_FLIGHT_TIME;
  if (apo > f.energy_apogee) why |= ERPL_WHY_ENERGY;
  return why;
}

// Edge i of np.linspace(lo, hi, bins + 1): two roundings, the last edge exact (erpl_mc_histogram's header comment).
struct ErplEdges {
  double lo, hi, delta, div, step;
  int bins;
  ERPL_TALLY_HD double operator[](int i) const {
    if (i >= bins) return hi;
    return step != 0.0 ? (double)i * step + lo : ((double)i / div) * delta + lo;
  }
};
ERPL_TALLY_HD ErplEdges erpl_edges_of(double lo, double hi, int bins) {
  ErplEdges e;
  e.lo = lo; e.hi = hi; e.bins = bins;
  e.delta = hi - lo; e.div = (double)bins; e.step = e.delta / e.div;
  return e;
}

// The bin of x in [lo, hi] among `bins` equal-width bins with edge values e[0..bins], as np.histogram finds it
// (_histograms_impl.py: f_indices, then one step down and one step up against the edges).  The clamps cannot act for x in
// [lo, hi]; they keep every read of e[] inside the row whatever the arithmetic does.  E: an array of the edges or ErplEdges.
template <class E>
ERPL_TALLY_HD int erpl_bin_of(double x, double lo, double hi, int bins, const E& e) {
  const double f = ((x - lo) / (hi - lo)) * (double)bins;
  int k = f >= (double)bins ? bins - 1 : (f > 0.0 ? (int)f : 0);
  if (x < e[k] && k > 0) k -= 1;
  if (k < bins - 1 && x >= e[k + 1]) k += 1;
  return k;
}

// One edge (xj, yj) -> (xi, yi) of a polygon against the sample (px, py): true if the sample changes sides
// (erpl_mc_impact_density's header comment; every operation rounded on its own).
ERPL_TALLY_HD bool erpl_zone_flips(double px, double py, double xi, double yi, double xj, double yj) {
  if ((yi > py) != (yj > py)) return px < (xj - xi) * (py - yi) / (yj - yi) + xi;
  return false;
}

// ---------------------------------------------------------------- the layout

struct ErplTallyLayout {
  int64_t row[ERPL_TALLY_MAX_ROWS], hist[ERPL_TALLY_MAX_ROWS], acc[ERPL_TALLY_MAX_ROWS], ext[ERPL_TALLY_MAX_ROWS];
  int64_t grid, cells, words;
};
// words of the extremes of one row: two counts, then (bits, id) per held value and side
ERPL_TALLY_HD int64_t erpl_tally_ext_words(int k) { return 2 + 4 * (int64_t)k; }

// the spec has been checked (erpl_tally_check_spec)
ERPL_TALLY_HD ErplTallyLayout erpl_tally_layout(const erpl_tally_spec& s) {
  ErplTallyLayout L;
  int64_t at = ERPL_TALLY_HEADER_WORDS;
  for (int j = 0; j < ERPL_TALLY_MAX_ROWS; ++j) {
    L.row[j] = L.hist[j] = L.acc[j] = L.ext[j] = at;
    if (j >= s.n_rows) continue;
    at += ERPL_TALLY_ROW_WORDS;
    L.hist[j] = at; at += s.bins[j];
    L.acc[j] = at; at += 2 * ERPL_TALLY_ACC_WORDS;
    L.ext[j] = at; at += erpl_tally_ext_words(s.k);
  }
  L.grid = at; at += ERPL_TALLY_GRID_WORDS;
  L.cells = at; at += (int64_t)s.bins_x * s.bins_y;
  L.words = at;
  return L;
}

// The refusals of a spec, in the order of the header.  Returns 0, or a code > 0 with *at = the index it concerns (-1: none);
// the text is the caller's (erpl_tally.hip) - this header knows no error buffer.
enum {
  ERPL_TALLY_BAD_BOUND = 1, ERPL_TALLY_BAD_N_ROWS, ERPL_TALLY_BAD_ROW, ERPL_TALLY_ROW_TWICE, ERPL_TALLY_BAD_BINS,
  ERPL_TALLY_BAD_RANGE, ERPL_TALLY_BAD_CENTRE, ERPL_TALLY_BAD_N_THRESHOLDS, ERPL_TALLY_BAD_THRESHOLD, ERPL_TALLY_BAD_K,
  ERPL_TALLY_BAD_N_Q, ERPL_TALLY_BAD_Q, ERPL_TALLY_BAD_ROW_X, ERPL_TALLY_BAD_ROW_Y, ERPL_TALLY_ROW_XY_SAME,
  ERPL_TALLY_BAD_BINS_X, ERPL_TALLY_BAD_BINS_Y, ERPL_TALLY_BAD_RANGE_X, ERPL_TALLY_BAD_RANGE_Y, ERPL_TALLY_BAD_N_ZONES,
  ERPL_TALLY_BAD_ZONE_FIRST, ERPL_TALLY_ZONE_SHORT, ERPL_TALLY_ZONE_LONG, ERPL_TALLY_BAD_VERTEX
};
inline bool erpl_tally_range_ok(double lo, double hi) {
  return erpl_is_finite(lo) && erpl_is_finite(hi) && erpl_is_finite(hi - lo) && lo < hi;
}
inline int erpl_tally_check_spec(const erpl_tally_spec& s, int* at) {
  *at = -1;
  const double bound[5] = {s.max_apogee, s.min_apogee, s.max_range, s.max_flight_time, s.energy_apogee};
  for (int b = 0; b < 5; ++b)
    if (bound[b] != bound[b]) { *at = b; return ERPL_TALLY_BAD_BOUND; }
  if (s.n_rows < 0 || s.n_rows > ERPL_TALLY_MAX_ROWS) return ERPL_TALLY_BAD_N_ROWS;
  for (int j = 0; j < s.n_rows; ++j) {
    *at = j;
    if (s.rows[j] < 0 || s.rows[j] >= ERPL_SUMMARY_DIM) return ERPL_TALLY_BAD_ROW;
    for (int i = 0; i < j; ++i)
      if (s.rows[i] == s.rows[j]) return ERPL_TALLY_ROW_TWICE;
  }
  for (int j = 0; j < s.n_rows; ++j) {
    *at = j;
    if (s.bins[j] < 1 || s.bins[j] > ERPL_TALLY_MAX_BINS) return ERPL_TALLY_BAD_BINS;
    if (!erpl_tally_range_ok(s.lo[j], s.hi[j])) return ERPL_TALLY_BAD_RANGE;
    if (!erpl_is_finite(s.centre[j])) return ERPL_TALLY_BAD_CENTRE;
    if (s.n_thresholds[j] < 0 || s.n_thresholds[j] > ERPL_TALLY_MAX_THRESHOLDS) return ERPL_TALLY_BAD_N_THRESHOLDS;
    for (int t = 0; t < s.n_thresholds[j]; ++t)
      if (s.threshold[j][t] != s.threshold[j][t]) return ERPL_TALLY_BAD_THRESHOLD;
  }
  *at = -1;
  if (s.k < 0 || s.k > ERPL_TALLY_MAX_K) return ERPL_TALLY_BAD_K;
  if (s.n_q < 0 || s.n_q > ERPL_TALLY_MAX_Q) return ERPL_TALLY_BAD_N_Q;
  for (int q = 0; q < s.n_q; ++q)
    if (!(s.q[q] >= 0.0 && s.q[q] <= 1.0)) { *at = q; return ERPL_TALLY_BAD_Q; }
  if (s.row_x < 0 || s.row_x >= ERPL_SUMMARY_DIM) return ERPL_TALLY_BAD_ROW_X;
  if (s.row_y < 0 || s.row_y >= ERPL_SUMMARY_DIM) return ERPL_TALLY_BAD_ROW_Y;
  if (s.row_x == s.row_y) return ERPL_TALLY_ROW_XY_SAME;
  if (s.bins_x < 1 || s.bins_x > ERPL_TALLY_MAX_GRID) return ERPL_TALLY_BAD_BINS_X;
  if (s.bins_y < 1 || s.bins_y > ERPL_TALLY_MAX_GRID) return ERPL_TALLY_BAD_BINS_Y;
  if (!erpl_tally_range_ok(s.lo_x, s.hi_x)) return ERPL_TALLY_BAD_RANGE_X;
  if (!erpl_tally_range_ok(s.lo_y, s.hi_y)) return ERPL_TALLY_BAD_RANGE_Y;
  if (s.n_zones < 0 || s.n_zones > ERPL_TALLY_MAX_ZONES) return ERPL_TALLY_BAD_N_ZONES;
  if (s.n_zones > 0 && s.zone_first[0] != 0) { *at = 0; return ERPL_TALLY_BAD_ZONE_FIRST; }
  for (int z = 0; z < s.n_zones; ++z) {
    *at = z;
    const int first = s.zone_first[z], end = s.zone_first[z + 1];
    if (end < first) return ERPL_TALLY_BAD_ZONE_FIRST;
    if (end - first < 3) return ERPL_TALLY_ZONE_SHORT;
    if (end > ERPL_TALLY_MAX_VERTICES) return ERPL_TALLY_ZONE_LONG;
    for (int v = first; v < end; ++v)
      if (!(erpl_is_finite(s.zone_x[v]) && erpl_is_finite(s.zone_y[v]))) { *at = v; return ERPL_TALLY_BAD_VERTEX; }
  }
  *at = -1;
  return 0;
}

// ---------------------------------------------------------------- the long accumulator

// The parts of a finite double v, |v| < 2^1000: v = (c[0] + c[1] 2^32 + c[2] 2^64) 2^(32 j - 1088), |c[i]| < 2^32.
struct ErplAccParts {
  int j;
  int64_t c[3];
};
ERPL_TALLY_HD ErplAccParts erpl_acc_split(double v) {
  const uint64_t b = erpl_bits_of(v);
  const int ef = (int)((b >> 52) & 0x7ffu);
  uint64_t m = b & 0x000fffffffffffffull;
  int e = -1074;
  if (ef != 0) { m |= 1ull << 52; e = ef - 1075; }
  ErplAccParts p;
  const int pos = e + ERPL_TALLY_ACC_BIAS, s = pos & 31;
  p.j = pos >> 5;
  const uint64_t low = m << s, high = s ? m >> (64 - s) : 0ull;   // m < 2^53, s < 32: high < 2^21
  p.c[0] = (int64_t)(low & 0xffffffffull);
  p.c[1] = (int64_t)(low >> 32);
  p.c[2] = (int64_t)high;
  if (b >> 63) { p.c[0] = -p.c[0]; p.c[1] = -p.c[1]; p.c[2] = -p.c[2]; }
  return p;
}

// carries from digit `from` upwards until the form is canonical again (all of them: from = 0)
ERPL_TALLY_HD void erpl_acc_normalise(int64_t* w, int from = 0) {
  for (int i = from; i < ERPL_TALLY_ACC_WORDS - 1; ++i) {
    const int64_t low = w[i] & 0xffffffffll;
    const int64_t carry = (w[i] - low) / 4294967296ll;   // exact: the difference is a multiple of 2^32
    w[i] = low;
    w[i + 1] += carry;
  }
}

// what a counted value adds to the two accumulators of its row; false: |d| is too large, the sample counts in moment_skipped
struct ErplMoment {
  double d, hi, lo;
};
ERPL_TALLY_HD bool erpl_tally_moment(double x, double centre, ErplMoment* m) {
  const double d = x - centre;
  if (!(fabs(d) < 0x1p500)) return false;
  m->d = d;
  m->hi = d * d;
  m->lo = fabs(d) < 0x1p-485 ? 0.0 : fma(d, d, -m->hi);
  return true;
}

// ---------------------------------------------------------------- extremes

// an entry of a held list: the sort key of its side (smallest: key, largest: ~key) and the id
struct ErplExtreme {
  uint64_t key;
  int64_t id;
};
ERPL_TALLY_HD bool erpl_extreme_before(const ErplExtreme& a, const ErplExtreme& b) {
  return a.key < b.key || (a.key == b.key && a.id < b.id);
}
ERPL_TALLY_HD uint64_t erpl_extreme_key(double v, int side) { return side ? ~erpl_tally_key(v) : erpl_tally_key(v); }
ERPL_TALLY_HD uint64_t erpl_extreme_bits(uint64_t key, int side) { return erpl_tally_bits_of_key(side ? ~key : key); }

// true: word w of a state belongs to the extremes of some row (merged by the sort, not by addition)
ERPL_TALLY_HD bool erpl_tally_is_extreme(const ErplTallyLayout& L, int n_rows, int k, int64_t w) {
  for (int j = 0; j < n_rows; ++j)
    if (w >= L.ext[j] && w < L.ext[j] + erpl_tally_ext_words(k)) return true;
  return false;
}

// ---------------------------------------------------------------- the host side: add, merge, result

// one value into a sorted held list of at most k entries ((bits, id) pairs at `list`, *held of them in use)
inline void erpl_tally_hold(int64_t* list, int64_t* held, int k, int side, double v, int64_t id) {
  if (k <= 0) return;
  ErplExtreme in = {erpl_extreme_key(v, side), id};
  int64_t n = *held;
  if (n == k) {
    const ErplExtreme last = {erpl_extreme_key(erpl_double_of((uint64_t)list[2 * (n - 1)]), side), list[2 * (n - 1) + 1]};
    if (!erpl_extreme_before(in, last)) return;
    n -= 1;   // the last one leaves
  }
  int64_t at = n;
  while (at > 0) {
    const ErplExtreme prev = {erpl_extreme_key(erpl_double_of((uint64_t)list[2 * (at - 1)]), side), list[2 * (at - 1) + 1]};
    if (!erpl_extreme_before(in, prev)) break;
    list[2 * at] = list[2 * (at - 1)];
    list[2 * at + 1] = list[2 * (at - 1) + 1];
    at -= 1;
  }
  list[2 * at] = (int64_t)erpl_bits_of(v);
  list[2 * at + 1] = id;
  *held = n + 1;
}

inline void erpl_acc_add(int64_t* w, double v) {
  const ErplAccParts p = erpl_acc_split(v);
  for (int i = 0; i < 3; ++i) w[p.j + i] += p.c[i];
  erpl_acc_normalise(w, p.j);
}

// summary [16][ld], status [n] or NULL; spec checked, n >= 1
inline void erpl_tally_add_rule(const erpl_tally_spec& s, int64_t* state, const double* summary, int64_t ld, const int32_t* status,
                                int64_t n, int64_t first_id) {
  const ErplTallyLayout L = erpl_tally_layout(s);
  const ErplFilter f = {s.max_apogee, s.min_apogee, s.max_range, s.max_flight_time, s.energy_apogee};
  ErplEdges edges[ERPL_TALLY_MAX_ROWS];
  for (int j = 0; j < s.n_rows; ++j) edges[j] = erpl_edges_of(s.lo[j], s.hi[j], s.bins[j]);
  const ErplEdges ex = erpl_edges_of(s.lo_x, s.hi_x, s.bins_x), ey = erpl_edges_of(s.lo_y, s.hi_y, s.bins_y);
  state[0] += n;
  for (int64_t i = 0; i < n; ++i) {
    const int why = erpl_why_of(f, summary[ERPL_SUM_APOGEE_ALT * ld + i], summary[ERPL_SUM_RANGE * ld + i],
                                summary[ERPL_SUM_FLIGHT_TIME * ld + i]);
    for (int b = 0; b < 6; ++b) state[2 + b] += (why >> b) & 1;
    if (status) {
      const int32_t st = status[i];
      if ((st & 0xFF) < 5) state[8 + (st & 0xFF)] += 1;
      if (st & ERPL_ST_NAN) state[13] += 1;
      if (st & ERPL_ST_INCOMPLETE) state[14] += 1;
    }
    if (why != 0) continue;
    state[1] += 1;
    for (int j = 0; j < s.n_rows; ++j) {
      const double x = summary[(int64_t)s.rows[j] * ld + i];
      if (!erpl_is_finite(x)) continue;
      int64_t* row = state + L.row[j];
      row[0] += 1;
      if (x < s.lo[j]) row[1] += 1;
      else if (x > s.hi[j]) row[2] += 1;
      else state[L.hist[j] + erpl_bin_of(x, s.lo[j], s.hi[j], s.bins[j], edges[j])] += 1;
      for (int t = 0; t < s.n_thresholds[j]; ++t)
        if (x > s.threshold[j][t]) row[4 + t] += 1;
      ErplMoment m;
      if (erpl_tally_moment(x, s.centre[j], &m)) {
        erpl_acc_add(state + L.acc[j], m.d);
        erpl_acc_add(state + L.acc[j] + ERPL_TALLY_ACC_WORDS, m.hi);
        erpl_acc_add(state + L.acc[j] + ERPL_TALLY_ACC_WORDS, m.lo);
      } else {
        row[3] += 1;
      }
      int64_t* ext = state + L.ext[j];
      erpl_tally_hold(ext + 2, ext + 0, s.k, 0, x, first_id + i);
      erpl_tally_hold(ext + 2 + 2 * s.k, ext + 1, s.k, 1, x, first_id + i);
    }
    const double px = summary[(int64_t)s.row_x * ld + i], py = summary[(int64_t)s.row_y * ld + i];
    if (!erpl_is_finite(px) || !erpl_is_finite(py)) continue;
    int64_t* grid = state + L.grid;
    grid[0] += 1;
    if (px >= s.lo_x && px <= s.hi_x && py >= s.lo_y && py <= s.hi_y)
      state[L.cells + (int64_t)erpl_bin_of(px, s.lo_x, s.hi_x, s.bins_x, ex) * s.bins_y + erpl_bin_of(py, s.lo_y, s.hi_y, s.bins_y, ey)] += 1;
    else
      grid[1] += 1;
    for (int z = 0; z < s.n_zones; ++z) {
      const int v0 = s.zone_first[z], v1 = s.zone_first[z + 1];
      bool c = false;
      for (int vi = v0, vj = v1 - 1; vi < v1; vj = vi++)
        if (erpl_zone_flips(px, py, s.zone_x[vi], s.zone_y[vi], s.zone_x[vj], s.zone_y[vj])) c = !c;
      if (c) grid[2 + z] += 1;
    }
  }
}

inline void erpl_tally_merge_rule(const erpl_tally_spec& s, int64_t* dst, const int64_t* src) {
  const ErplTallyLayout L = erpl_tally_layout(s);
  for (int64_t w = 0; w < L.words; ++w)
    if (!erpl_tally_is_extreme(L, s.n_rows, s.k, w)) dst[w] += src[w];
  for (int j = 0; j < s.n_rows; ++j) {
    erpl_acc_normalise(dst + L.acc[j]);
    erpl_acc_normalise(dst + L.acc[j] + ERPL_TALLY_ACC_WORDS);
    for (int side = 0; side < 2; ++side) {
      const int64_t* from = src + L.ext[j] + 2 + 2 * s.k * side;
      const int64_t held = src[L.ext[j] + side];
      for (int64_t e = 0; e < held && e < s.k; ++e)
        erpl_tally_hold(dst + L.ext[j] + 2 + 2 * s.k * side, dst + L.ext[j] + side, s.k, side, erpl_double_of((uint64_t)from[2 * e]),
                        from[2 * e + 1]);
    }
  }
}

// a canonical accumulator rounded once to the nearest double, ties to even
inline double erpl_acc_round(const int64_t* w) {
  uint32_t mag[ERPL_TALLY_ACC_WORDS];
  const bool neg = w[ERPL_TALLY_ACC_WORDS - 1] < 0;
  uint64_t carry = neg ? 1u : 0u;
  for (int i = 0; i < ERPL_TALLY_ACC_WORDS; ++i) {   // |value|: two's complement negation over the digits
    const uint32_t digit = (uint32_t)(uint64_t)w[i];
    const uint64_t t = (uint64_t)(neg ? ~digit : digit) + carry;
    mag[i] = (uint32_t)t;
    carry = neg ? t >> 32 : 0u;
  }
  int top = ERPL_TALLY_ACC_WORDS - 1;
  while (top >= 0 && mag[top] == 0u) --top;
  if (top < 0) return 0.0;
  int lead = 31;
  while (!((mag[top] >> lead) & 1u)) --lead;
  const int64_t high = 32 * (int64_t)top + lead;   // the leading bit, counted from bit 0 of digit 0
  auto bit = [&](int64_t p) -> uint64_t { return p < 0 ? 0u : (mag[p >> 5] >> (p & 31)) & 1u; };
  uint64_t m = 0;
  for (int t = 0; t < 53; ++t) m = (m << 1) | bit(high - t);
  const uint64_t half = bit(high - 53);
  bool sticky = false;
  for (int64_t p = high - 54; p >= 0 && !sticky; --p) sticky = bit(p) != 0u;
  if (half && (sticky || (m & 1u))) m += 1;
  const double v = ldexp((double)m, (int)(high - 52 - ERPL_TALLY_ACC_BIAS));
  return neg ? -v : v;
}

// value of order statistic r (0-based) of row j if it is held, with *held = true
inline double erpl_tally_order(const int64_t* ext, int k, int64_t count, int64_t r, bool* held) {
  const int64_t n_lo = ext[0], n_hi = ext[1];
  *held = true;
  if (r < n_lo) return erpl_double_of((uint64_t)ext[2 + 2 * r]);
  if (r >= count - n_hi) return erpl_double_of((uint64_t)ext[2 + 2 * k + 2 * (count - 1 - r)]);
  *held = false;
  return NAN;
}

// where order statistic r lies by the histogram: NaN in the below / above mass
inline double erpl_tally_order_binned(const int64_t* row, const int64_t* hist, const ErplEdges& e, int64_t r) {
  if (r < row[1]) return NAN;
  int64_t before = row[1];
  for (int b = 0; b < e.bins; ++b) {
    const int64_t c = hist[b];
    if (r < before + c) return e[b] + (e[b + 1] - e[b]) * (((double)(r - before) + 0.5) / (double)c);
    before += c;
  }
  return NAN;
}

// 0, or 1: a count word has passed 2^62
inline int erpl_tally_result_rule(const erpl_tally_spec& s, const int64_t* state, erpl_tally* out, int64_t* hist_counts,
                                  int64_t* grid_counts) {
  const ErplTallyLayout L = erpl_tally_layout(s);
  const int64_t most = (int64_t)1 << 62;
  for (int64_t w = 0; w < L.words; ++w) {
    bool counts = !erpl_tally_is_extreme(L, s.n_rows, s.k, w);
    for (int j = 0; j < s.n_rows; ++j)
      if (w >= L.acc[j] && w < L.acc[j] + 2 * ERPL_TALLY_ACC_WORDS) counts = false;
    if (counts && (state[w] < 0 || state[w] > most)) return 1;
  }
  memset(out, 0, sizeof(*out));
  out->n = state[0]; out->n_valid = state[1]; out->n_outliers = state[0] - state[1];
  for (int b = 0; b < 6; ++b) out->reason_counts[b] = state[2 + b];
  for (int b = 0; b < 5; ++b) out->termination_counts[b] = state[8 + b];
  out->n_status_nan = state[13]; out->n_incomplete = state[14];
  out->grid_counted = state[L.grid]; out->grid_outside = state[L.grid + 1];
  for (int z = 0; z < ERPL_TALLY_MAX_ZONES; ++z) out->zone_inside[z] = z < s.n_zones ? state[L.grid + 2 + z] : 0;
  if (grid_counts) memcpy(grid_counts, state + L.cells, (size_t)s.bins_x * s.bins_y * sizeof(int64_t));
  if (hist_counts) memset(hist_counts, 0, (size_t)ERPL_TALLY_MAX_ROWS * ERPL_TALLY_MAX_BINS * sizeof(int64_t));
  for (int j = 0; j < ERPL_TALLY_MAX_ROWS; ++j) {
    erpl_tally_row& o = out->row[j];
    o.sum_d = o.sum_d2 = o.mean = o.var = o.std = o.min = o.max = NAN;
    for (int q = 0; q < ERPL_TALLY_MAX_Q; ++q) o.quantile[q] = NAN;
    if (j >= s.n_rows) continue;
    const int64_t* row = state + L.row[j];
    const int64_t* hist = state + L.hist[j];
    const int64_t* ext = state + L.ext[j];
    if (hist_counts) memcpy(hist_counts + (size_t)j * ERPL_TALLY_MAX_BINS, hist, (size_t)s.bins[j] * sizeof(int64_t));
    o.count = row[0]; o.below = row[1]; o.above = row[2]; o.moment_skipped = row[3];
    for (int t = 0; t < s.n_thresholds[j]; ++t) o.exceed[t] = row[4 + t];
    o.n_smallest = (int32_t)ext[0]; o.n_largest = (int32_t)ext[1];
    for (int e = 0; e < o.n_smallest; ++e) {
      o.smallest[e].value = erpl_double_of((uint64_t)ext[2 + 2 * e]);
      o.smallest[e].id = ext[2 + 2 * e + 1];
    }
    for (int e = 0; e < o.n_largest; ++e) {
      o.largest[e].value = erpl_double_of((uint64_t)ext[2 + 2 * s.k + 2 * e]);
      o.largest[e].id = ext[2 + 2 * s.k + 2 * e + 1];
    }
    o.sum_d = erpl_acc_round(state + L.acc[j]);
    o.sum_d2 = erpl_acc_round(state + L.acc[j] + ERPL_TALLY_ACC_WORDS);
    if (o.count <= 0) continue;
    const double cnt = (double)o.count;
    const double md = o.sum_d / cnt;
    o.mean = s.centre[j] + md;
    o.var = (o.sum_d2 - o.sum_d * md) / cnt;
    o.std = sqrt(o.var);
    if (o.n_smallest > 0) o.min = o.smallest[0].value;
    if (o.n_largest > 0) o.max = o.largest[0].value;
    const ErplEdges e = erpl_edges_of(s.lo[j], s.hi[j], s.bins[j]);
    for (int q = 0; q < s.n_q; ++q) {
      // np.percentile (linear): the virtual index, its two neighbours and NumPy's two-sided interpolation, op for op
      const double vi = (double)(o.count - 1) * s.q[q];
      int64_t r0, r1;
      double g = 0.0;
      if (vi >= (double)(o.count - 1)) r0 = r1 = o.count - 1;
      else if (vi < 0.0) r0 = r1 = 0;
      else { r0 = (int64_t)floor(vi); r1 = r0 + 1; g = vi - floor(vi); }
      bool held0, held1;
      double a = erpl_tally_order(ext, s.k, o.count, r0, &held0), b = erpl_tally_order(ext, s.k, o.count, r1, &held1);
      o.quantile_exact[q] = held0 && held1;
      if (!held0) a = erpl_tally_order_binned(row, hist, e, r0);
      if (!held1) b = erpl_tally_order_binned(row, hist, e, r1);
      const double diff = b - a;
      double v = a + diff * g;
      if (g >= 0.5) v = b - diff * (1.0 - g);
      o.quantile[q] = v;
    }
  }
  return 0;
}
