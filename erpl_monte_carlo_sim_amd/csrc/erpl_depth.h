// erpl_depth.h — the rules of erpl_mc_corridor_depth that exist once, for the kernels of erpl_corridor_depth.hip, the host half
// in erpl_stats_api.hip and the stand-alone erpl_depth_check: the pair count of a band depth, the size of the central region,
// the fences, which path the rank pass of a row takes and how the call cuts its device buffer into pieces.  No HIP: plain
// C++ that hipcc compiles for both sides.  Internal, never installed.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "erpl_mc.h"

#ifdef __HIPCC__
#define ERPL_DEPTH_HD __host__ __device__
#else
#define ERPL_DEPTH_HD
#endif

// ERPL_DEPTH_LDS_MAX (erpl_mc.h) is the built-in limit of the LDS path of the rank pass: a row of up to that many columns is
// sorted by one workgroup in LDS (the next power of two of 8-byte keys: 128 KB at the limit, which the 160 KB of a gfx950 CU
// hold).  spec.lds_limit lowers it.
// the least and the most threads of a workgroup of the LDS path
#define ERPL_DEPTH_LDS_MIN_THREADS 64
#define ERPL_DEPTH_LDS_MAX_THREADS 1024
// Global path: rows of up to this many columns are sorted as the segments of one segmented sort per group of rows, longer
// rows by one device-wide sort each (a segment is sorted by one workgroup).  Measured on (3, 256, m), DESIGN.md section 8.22: at
// 131 072 columns the segmented sort takes 13.6 ms of sort kernels against 47.0 ms for a sort per row, at 262 144 it takes 52.1 ms.
#define ERPL_DEPTH_SEG_MAX 131072
// the keys of a group of rows of the global path, in and out together, take at most this many bytes (one row at the least)
#define ERPL_DEPTH_KEY_BYTES ((size_t)512 << 20)
// the pair of a column outside its row's population
#define ERPL_DEPTH_NONE 0xffffffffu

// C2(n) = n (n - 1) / 2, the pairs among n members.  n < 2^31: below 2^61.
ERPL_DEPTH_HD inline int64_t erpl_depth_c2(int64_t n) { return n * (n - 1) / 2; }

// The pairs of members of a population of n - pairs with the member itself included - whose band [min, max] contains a member
// with a members strictly below it and b strictly above it: every pair but those that lie on one side of it.
ERPL_DEPTH_HD inline int64_t erpl_depth_cov(int64_t n, int64_t a, int64_t b) {
  return erpl_depth_c2(n) - erpl_depth_c2(a) - erpl_depth_c2(b);
}

// The terms a counted node (n >= 2) adds to the two sums of a column: cov / C2(n) and (n - a) / n, one IEEE division each.
ERPL_DEPTH_HD inline double erpl_depth_term(int64_t n, int64_t a, int64_t b) {
  return (double)erpl_depth_cov(n, a, b) / (double)erpl_depth_c2(n);
}
ERPL_DEPTH_HD inline double erpl_depth_mei_term(int64_t n, int64_t a) { return (double)(n - a) / (double)n; }

// h: the central region holds the h deepest of n_defined columns (and every column tied with the h-th).
// ceil(central * n_defined) in double, clamped to [1, n_defined]; 0 with nothing defined.
ERPL_DEPTH_HD inline int64_t erpl_depth_h(double central, int64_t n_defined) {
  if (n_defined <= 0) return 0;
  const double want = ceil(central * (double)n_defined);
  if (!(want >= 1.0)) return 1;
  if (want >= (double)n_defined) return n_defined;
  return (int64_t)want;
}

// The fences of a row from the envelope [lo, hi] of its central members: one rounding per operation (the units that include
// this header are compiled without contraction).
ERPL_DEPTH_HD inline void erpl_depth_fences(double lo, double hi, double factor, double* fence_lo, double* fence_hi) {
  const double w = hi - lo;
  const double reach = factor * w;
  *fence_lo = lo - reach;
  *fence_hi = hi + reach;
}

// the limit in force: the built-in one, or a smaller positive spec.lds_limit
ERPL_DEPTH_HD inline int64_t erpl_depth_lds_limit(int32_t lds_limit) {
  return (lds_limit <= 0 || lds_limit > ERPL_DEPTH_LDS_MAX) ? ERPL_DEPTH_LDS_MAX : lds_limit;
}
// the path of the rank pass: rows of m columns are sorted in LDS
ERPL_DEPTH_HD inline bool erpl_depth_use_lds(int64_t m, int32_t lds_limit) { return m <= erpl_depth_lds_limit(lds_limit); }
// the keys of a workgroup of the LDS path: the next power of two of m, at least 2 * ERPL_DEPTH_LDS_MIN_THREADS
ERPL_DEPTH_HD inline int erpl_depth_lds_keys(int64_t m) {
  int n = 2 * ERPL_DEPTH_LDS_MIN_THREADS;
  while (n < m) n <<= 1;
  return n;
}
// its threads: a compare-exchange each, at most ERPL_DEPTH_LDS_MAX_THREADS
ERPL_DEPTH_HD inline int erpl_depth_lds_threads(int64_t m) {
  const int t = erpl_depth_lds_keys(m) / 2;
  return t > ERPL_DEPTH_LDS_MAX_THREADS ? ERPL_DEPTH_LDS_MAX_THREADS : t;
}
// rows of a group of the global path
ERPL_DEPTH_HD inline int erpl_depth_group_rows(int64_t m, int n_nodes) {
  const size_t fit = ERPL_DEPTH_KEY_BYTES / (16 * (size_t)m);
  return fit < 1 ? 1 : (fit > (size_t)n_nodes ? n_nodes : (int)fit);
}

// The device buffer of a call over C channels, T nodes, m columns; every piece starts at a multiple of 256 bytes.
//   pair   [T][m] (a, b) uint32 pairs of ONE channel's rows: the rank pass writes them, the accumulation reads them
//   rown   [T] int32: the population of every row of that channel
//   keys   global path: [2][group][m] u64, the keys of a group of rows before and behind the sort; always [2][m] at the least,
//          the depth keys of a channel before and behind the sort of the selection
//   offs   [group + 1] uint32: the ends of the segments
//   temp   the scratch of the sorts (temp_bytes, from the library's sizing calls)
//   chan   [C] records of 8 eight-byte words: n_defined, n_central, n_outliers, median, threshold, depth_max, 2 spare
//   rows   [C T] erpl_depth_row
//   count  4 u64: [0] the masked columns
struct ErplDepthLayout {
  size_t pair, rown, keys, offs, temp, chan, rows, count, need;
  int group;      // rows per group of the global path; 0 on the LDS path
  bool lds;
};
inline ErplDepthLayout erpl_depth_layout(int64_t m, int C, int T, int32_t lds_limit, size_t temp_bytes) {
  ErplDepthLayout l = {};
  size_t end = 0;
  auto take = [&end](size_t bytes) { const size_t at = end; end = (end + bytes + 255) / 256 * 256; return at; };
  const size_t um = (size_t)m, uT = (size_t)T, uC = (size_t)C;
  l.lds = erpl_depth_use_lds(m, lds_limit);
  l.group = l.lds ? 0 : erpl_depth_group_rows(m, T);
  const size_t g = l.group > 1 ? (size_t)l.group : 1;
  l.pair = take(uT * um * 8);
  l.rown = take(uT * 4);
  l.keys = take(2 * g * um * 8);
  l.offs = take((g + 1) * 4);
  l.temp = take(temp_bytes);
  l.chan = take(uC * 64);
  l.rows = take(uC * uT * sizeof(erpl_depth_row));
  l.count = take(32);
  l.need = end;
  return l;
}
