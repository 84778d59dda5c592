// erpl_tally_check — erpl_tally.h on the host alone (no HIP, no library): what must hold before the kernel runs anywhere.
//   layout     for a set of specs: the pieces of the state in the documented order, none overlapping, `words` the end
//   canonical  after every add of an adversarial stream (alternating huge and tiny values, cancellations to zero, subnormals,
//              the largest admitted magnitudes) both accumulators of a row are in canonical form, and a stream that sums to
//              zero leaves all-zero words
//   rounding   erpl_acc_round against sums that a double holds exactly
//   splits     a fixed table tallied in one add, one sample per add, the same in reverse, and as a merge tree of five uneven
//              pieces: four states of equal bytes
// Prints one line per check; exit status 1 on the first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_tally.h"

namespace {

int fail(const char* what, long long at) {
  printf("FAIL %s (at %lld)\n", what, at);
  return 1;
}

erpl_tally_spec base_spec() {
  erpl_tally_spec s;
  memset(&s, 0, sizeof(s));
  s.max_apogee = 80000.0; s.min_apogee = 100.0; s.max_range = 200000.0; s.max_flight_time = 600.0; s.energy_apogee = 88073.0;
  s.n_rows = 3;
  const int rows[3] = {ERPL_SUM_APOGEE_ALT, ERPL_SUM_RANGE, ERPL_SUM_MAX_SPEED};
  for (int j = 0; j < 3; ++j) {
    s.rows[j] = rows[j];
    s.bins[j] = 7 + 50 * j;
    s.lo[j] = 0.0; s.hi[j] = 1000.0 * (j + 1);
    s.centre[j] = 10.0 * j;
    s.n_thresholds[j] = j;
    for (int t = 0; t < j; ++t) s.threshold[j][t] = 100.0 * t;
  }
  s.k = 5;
  s.n_q = 1; s.q[0] = 0.5;
  s.row_x = ERPL_SUM_IMPACT_X; s.row_y = ERPL_SUM_IMPACT_Y;
  s.bins_x = 9; s.bins_y = 4;
  s.lo_x = s.lo_y = -500.0; s.hi_x = s.hi_y = 500.0;
  s.n_zones = 1;
  s.zone_first[0] = 0; s.zone_first[1] = 3;
  s.zone_x[0] = -100.0; s.zone_y[0] = -100.0; s.zone_x[1] = 200.0; s.zone_y[1] = 0.0; s.zone_x[2] = 0.0; s.zone_y[2] = 300.0;
  return s;
}

int check_layout(const erpl_tally_spec& s) {
  int at = 0;
  if (erpl_tally_check_spec(s, &at) != 0) return fail("spec refused", at);
  const ErplTallyLayout L = erpl_tally_layout(s);
  int64_t end = ERPL_TALLY_HEADER_WORDS;
  for (int j = 0; j < s.n_rows; ++j) {
    if (L.row[j] != end) return fail("row counts out of place", j);
    end += ERPL_TALLY_ROW_WORDS;
    if (L.hist[j] != end) return fail("bins out of place", j);
    end += s.bins[j];
    if (L.acc[j] != end) return fail("accumulators out of place", j);
    end += 2 * ERPL_TALLY_ACC_WORDS;
    if (L.ext[j] != end) return fail("extremes out of place", j);
    end += erpl_tally_ext_words(s.k);
    for (int64_t w = L.row[j]; w < end; ++w)
      if (erpl_tally_is_extreme(L, s.n_rows, s.k, w) != (w >= L.ext[j])) return fail("extremes range", w);
  }
  if (L.grid != end) return fail("grid counts out of place", -1);
  end += ERPL_TALLY_GRID_WORDS;
  if (L.cells != end) return fail("cells out of place", -1);
  end += (int64_t)s.bins_x * s.bins_y;
  if (L.words != end) return fail("words is not the end", -1);
  // int64 words: every piece is 8-byte aligned by construction
  printf("layout rows=%d k=%d grid=%dx%d words=%lld ok\n", s.n_rows, s.k, s.bins_x, s.bins_y, (long long)L.words);
  return 0;
}

bool canonical(const int64_t* w) {
  for (int i = 0; i < ERPL_TALLY_ACC_WORDS - 1; ++i)
    if (w[i] < 0 || w[i] > 0xffffffffll) return false;
  return w[ERPL_TALLY_ACC_WORDS - 1] == 0 || w[ERPL_TALLY_ACC_WORDS - 1] == -1;
}

int check_canonical() {
  const double big = 0x1.fffffffffffffp499, tiny = 0x1p-1074;
  const double v[] = {big, -big, tiny, -tiny, 1.0, -1.0, 0x1p-60, 1e300, -1e300, -0x1p-60, 0x1.fffffffffffffp999, -0x1.fffffffffffffp999,
                      0x1p-1022, -0x1p-1022, 0x1.8p-1060, -0x1.8p-1060, 3.0, -3.0, -0.0, 0.0, 0x1p32, -0x1p32, 0x1p31, -0x1p31};
  const int nv = (int)(sizeof(v) / sizeof(v[0]));
  int64_t w[ERPL_TALLY_ACC_WORDS] = {};
  // every prefix of the stream, forwards then in a scrambled order, is canonical; the whole (pairs that cancel) is zero
  for (int round = 0; round < 3; ++round)
    for (int t = 0; t < nv; ++t) {
      erpl_acc_add(w, v[round == 1 ? (t * 7) % nv : (round == 2 ? nv - 1 - t : t)]);
      if (!canonical(w)) return fail("accumulator not canonical", round * 100 + t);
    }
  for (int i = 0; i < ERPL_TALLY_ACC_WORDS; ++i)
    if (w[i] != 0) return fail("a stream that cancels leaves a word", i);
  // 2^20 adds of the largest square: the top digits take the growth
  for (int t = 0; t < (1 << 20); ++t) erpl_acc_add(w, 0x1.fffffffffffffp999);
  if (!canonical(w)) return fail("accumulator not canonical after 2^20 large adds", -1);
  for (int t = 0; t < (1 << 20); ++t) erpl_acc_add(w, -0x1.fffffffffffffp999);
  for (int i = 0; i < ERPL_TALLY_ACC_WORDS; ++i)
    if (w[i] != 0) return fail("2^20 large adds and their negatives leave a word", i);
  // the parts as the device adds them: all parts first, the carries once
  for (int t = 0; t < nv; ++t) {
    const ErplAccParts p = erpl_acc_split(v[t]);
    if (p.j < 0 || p.j + 2 >= ERPL_TALLY_ACC_WORDS) return fail("a part outside the accumulator", t);
    for (int i = 0; i < 3; ++i) w[p.j + i] += p.c[i];
  }
  erpl_acc_normalise(w);
  for (int i = 0; i < ERPL_TALLY_ACC_WORDS; ++i)
    if (w[i] != 0) return fail("parts added before one normalisation leave a word", i);
  printf("canonical %d values x 3 orders, 2^21 large adds ok\n", nv);
  return 0;
}

int check_rounding() {
  struct Case { double a, b, want; };
  const Case c[] = {{1.0, 0x1p-53, 1.0},                       // a tie: to even
                    {1.0, 0x1.8p-53, 0x1.0000000000001p0},     // above the tie
                    {0x1.0000000000001p0, 0x1p-53, 0x1.0000000000002p0},   // a tie: to even, upwards
                    {1e300, -1e300, 0.0},
                    {0x1p-1074, 0x1p-1074, 0x1p-1073},
                    {-1.0, -0x1.8p-53, -0x1.0000000000001p0},
                    {0x1.fffffffffffffp52, 0.5, 0x1p53}};
  for (size_t t = 0; t < sizeof(c) / sizeof(c[0]); ++t) {
    int64_t w[ERPL_TALLY_ACC_WORDS] = {};
    erpl_acc_add(w, c[t].a);
    erpl_acc_add(w, c[t].b);
    const double got = erpl_acc_round(w);
    if (erpl_bits_of(got) != erpl_bits_of(c[t].want)) return fail("erpl_acc_round", (long long)t);
  }
  printf("rounding %d cases ok\n", (int)(sizeof(c) / sizeof(c[0])));
  return 0;
}

// a fixed table [16][n]: a counter-based scramble, with outliers, non-finite values, ties and zeros of both signs mixed in
void fill_table(int64_t n, std::vector<double>& summary, std::vector<int32_t>& status) {
  summary.assign((size_t)ERPL_SUMMARY_DIM * n, 0.0);
  status.assign((size_t)n, 0);
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (int r = 0; r < ERPL_SUMMARY_DIM; ++r)
    for (int64_t i = 0; i < n; ++i) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      double v = (double)(x >> 11) * 0x1p-53;
      if (r == ERPL_SUM_APOGEE_ALT) v = 200.0 + 900.0 * v;
      else if (r == ERPL_SUM_RANGE) v = (double)((x >> 20) % 37) * 60.0;          // ties, and values on bin edges
      else if (r == ERPL_SUM_FLIGHT_TIME) v = 10.0 + 500.0 * v;
      else if (r == ERPL_SUM_MAX_SPEED) v = (x & 7) == 0 ? ((x & 8) ? -0.0 : 0.0) : 4000.0 * v - 500.0;
      else v = 1200.0 * v - 600.0;
      if ((x & 0x3ff) == 1) v = NAN;
      if ((x & 0x3ff) == 2) v = -INFINITY;
      if ((x & 0x3ff) == 3) v = 1e300;
      summary[(size_t)r * n + i] = v;
    }
  for (int64_t i = 0; i < n; ++i) status[(size_t)i] = (int32_t)(i % 5) | ((i % 97) == 0 ? ERPL_ST_NAN : 0);
}

int check_splits() {
  const erpl_tally_spec s = base_spec();
  const int64_t n = 1025, first_id = 1000000007;
  std::vector<double> summary;
  std::vector<int32_t> status;
  fill_table(n, summary, status);
  const size_t words = (size_t)erpl_tally_layout(s).words;
  std::vector<int64_t> one(words, 0), each(words, 0), back(words, 0), tree(words, 0);
  erpl_tally_add_rule(s, one.data(), summary.data(), n, status.data(), n, first_id);
  for (int64_t i = 0; i < n; ++i) erpl_tally_add_rule(s, each.data(), summary.data() + i, n, status.data() + i, 1, first_id + i);
  for (int64_t i = n - 1; i >= 0; --i) erpl_tally_add_rule(s, back.data(), summary.data() + i, n, status.data() + i, 1, first_id + i);
  const int64_t cut[6] = {0, 1, 64, 129, 700, n};
  std::vector<std::vector<int64_t>> piece(5, std::vector<int64_t>(words, 0));
  for (int p = 0; p < 5; ++p)
    erpl_tally_add_rule(s, piece[p].data(), summary.data() + cut[p], n, status.data() + cut[p], cut[p + 1] - cut[p], first_id + cut[p]);
  erpl_tally_merge_rule(s, piece[3].data(), piece[4].data());   // ((3 + 4) + 1) and (0 + 2), then both into the empty tally
  erpl_tally_merge_rule(s, piece[3].data(), piece[1].data());
  erpl_tally_merge_rule(s, piece[0].data(), piece[2].data());
  erpl_tally_merge_rule(s, tree.data(), piece[3].data());
  erpl_tally_merge_rule(s, tree.data(), piece[0].data());
  if (memcmp(one.data(), each.data(), words * 8) != 0) return fail("one add != one sample per add", -1);
  if (memcmp(one.data(), back.data(), words * 8) != 0) return fail("one add != one sample per add, reversed", -1);
  if (memcmp(one.data(), tree.data(), words * 8) != 0) return fail("one add != merge tree of five pieces", -1);
  const ErplTallyLayout L = erpl_tally_layout(s);
  for (int j = 0; j < s.n_rows; ++j)
    if (!canonical(one.data() + L.acc[j]) || !canonical(one.data() + L.acc[j] + ERPL_TALLY_ACC_WORDS)) return fail("state accumulator not canonical", j);
  erpl_tally r;
  std::vector<int64_t> hist((size_t)ERPL_TALLY_MAX_ROWS * ERPL_TALLY_MAX_BINS), cells((size_t)s.bins_x * s.bins_y);
  if (erpl_tally_result_rule(s, one.data(), &r, hist.data(), cells.data()) != 0) return fail("result refused", -1);
  for (int j = 0; j < s.n_rows; ++j) {
    int64_t in = 0;
    for (int b = 0; b < s.bins[j]; ++b) in += hist[(size_t)j * ERPL_TALLY_MAX_BINS + b];
    if (in + r.row[j].below + r.row[j].above != r.row[j].count) return fail("bins + below + above != count", j);
    if (r.row[j].n_smallest != (r.row[j].count < s.k ? r.row[j].count : s.k)) return fail("held smallest", j);
  }
  int64_t in = 0;
  for (int64_t v : cells) in += v;
  if (in + r.grid_outside != r.grid_counted) return fail("cells + outside != counted", -1);
  printf("splits n=%lld valid=%lld counted=%lld/%lld/%lld zone=%lld: one add = 1025 adds = reversed = merge tree, %zu words ok\n", (long long)r.n,
         (long long)r.n_valid, (long long)r.row[0].count, (long long)r.row[1].count, (long long)r.row[2].count, (long long)r.zone_inside[0], words);
  return 0;
}

}  // namespace

int main() {
  erpl_tally_spec s = base_spec();
  if (check_layout(s)) return 1;
  s.n_rows = 0; s.k = 0; s.bins_x = 256; s.bins_y = 256; s.n_zones = 0;
  if (check_layout(s)) return 1;
  s = base_spec();
  s.n_rows = 1; s.bins[0] = 1024; s.k = 64; s.bins_x = 1; s.bins_y = 1;
  if (check_layout(s)) return 1;
  if (check_canonical()) return 1;
  if (check_rounding()) return 1;
  if (check_splits()) return 1;
  printf("erpl_tally_check ok\n");
  return 0;
}
