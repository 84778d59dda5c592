// erpl_design_check — erpl_design.h on the host alone (no HIP, no library): fills the shapes the tests use and checks what
// must hold before the kernel runs anywhere.  For every shape (rows, n, block, first, count, first_row) and the kinds LHS and
// LHS_CENTRED: every row of every replicate hits each of its m strata exactly once (the permutation is a bijection and p
// stays in its stratum), every p lies strictly inside (0, 1), every normal value is finite, and the window
// [first, first + count) equals those columns of the full rows bit for bit.  Prints one line per shape; exit status 1 on the
// first violation.  Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_design.h"

namespace {
struct Shape {
  int rows;
  int64_t n, block, first, count;
  int first_row;
};

const Shape kShapes[] = {{3, 1, 0, 0, 1, 0},        {4, 2, 0, 0, 2, 0},          {5, 5, 0, 0, 5, 0},
                         {5, 17, 0, 0, 17, 0},      {7, 64, 0, 0, 64, 0},        {23, 65, 0, 0, 65, 0},
                         {23, 4097, 0, 1, 4095, 0}, {8, 65537, 0, 65000, 537, 0}, {2, 1000003, 0, 995907, 4096, 0},
                         {6, 4096, 512, 300, 1000, 0}, {5, 300, 0, 0, 300, 314},  {64, 4096, 0, 0, 4096, 0},
                         {64, 5000, 0, 0, 5000, 0},  {64, 257, 0, 0, 257, 0},     {20, 256, 0, 0, 256, 0}};

// row r of the call, columns [first, first + count) of the design, into out[count]
bool fill(uint64_t seed, int kind, bool normal, const Shape& s, int r, int64_t first, int64_t count, double* out) {
  const uint32_t m = (uint32_t)(s.block ? s.block : s.n), b = erpl_design_half_bits(m), g = (uint32_t)(s.first_row + r);
  bool capped = false;
  ErplDesignKeys K = {};
  int64_t have = -1;
  for (int64_t c = 0; c < count; ++c) {
    const uint32_t i = (uint32_t)(first + c), rho = i / m, l = i - rho * m;
    if (have != (int64_t)rho) { K = erpl_design_keys(seed, g, rho); have = rho; }
    out[c] = erpl_design_value(seed, kind, normal, g, i, K.k, b, m, l, &capped);
  }
  return !capped;
}
}  // namespace

int main() {
  const uint64_t seed = 7;
  for (const Shape& s : kShapes) {
    const uint32_t m = (uint32_t)(s.block ? s.block : s.n);
    std::vector<double> full((size_t)s.n), win((size_t)s.count), z((size_t)s.count);
    std::vector<char> seen(m);
    for (int kind = ERPL_DESIGN_LHS; kind <= ERPL_DESIGN_LHS_CENTRED; ++kind)
      for (int r = 0; r < s.rows; ++r) {
        if (!fill(seed, kind, false, s, r, 0, s.n, full.data()) || !fill(seed, kind, false, s, r, s.first, s.count, win.data()) ||
            !fill(seed, kind, true, s, r, s.first, s.count, z.data())) {
          printf("FAIL n=%lld row=%d: a cycle walk reached the cap\n", (long long)s.n, r);
          return 1;
        }
        if (memcmp(win.data(), full.data() + s.first, (size_t)s.count * sizeof(double)) != 0) {
          printf("FAIL n=%lld row=%d: the window differs from the full row\n", (long long)s.n, r);
          return 1;
        }
        for (int64_t rep = 0; rep < s.n / m; ++rep) {
          memset(seen.data(), 0, seen.size());
          for (uint32_t l = 0; l < m; ++l) {
            const double p = full[(size_t)(rep * m + l)];
            uint32_t k = (uint32_t)(p * (double)m);
            if (k > 0 && p < (double)k / (double)m) --k;   // p * m rounded up to the next stratum's edge
            if (!(p > 0.0 && p < 1.0) || k >= m || seen[k]) {
              printf("FAIL n=%lld row=%d replicate=%lld: stratum %u hit twice or p = %a outside (0, 1)\n", (long long)s.n, r,
                     (long long)rep, k, p);
              return 1;
            }
            seen[k] = 1;
          }
        }
        for (int64_t c = 0; c < s.count; ++c)
          if (!isfinite(z[(size_t)c])) {
            printf("FAIL n=%lld row=%d: normal value %lld is not finite\n", (long long)s.n, r, (long long)c);
            return 1;
          }
      }
    printf("ok rows=%d n=%lld block=%lld first=%lld count=%lld first_row=%d\n", s.rows, (long long)s.n, (long long)s.block,
           (long long)s.first, (long long)s.count, s.first_row);
  }
  return 0;
}
