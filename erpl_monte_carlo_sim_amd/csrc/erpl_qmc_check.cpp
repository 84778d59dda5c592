// erpl_qmc_check — erpl_qmc.h on the host alone (no HIP, no library): expands the table and checks what must hold before the
// kernel runs anywhere.  The table gives exactly ERPL_QMC_MAX_DIMS dimensions and every V[d][j] has bit 31 - j set and none
// below it (the generating matrices are upper triangular with a unit diagonal).  For every shape (rows, n, block, first,
// count, first_row) under RAW and OWEN, with the dimensions of dims == NULL: every p lies strictly inside (0, 1), every
// normal value is finite, the window [first, first + count) equals those columns of the full rows bit for bit, and, where the
// full rows are affordable, every aligned block of 2^k columns of a replicate puts one p into each interval of width 2^-k.
// Under OWEN the first 256 columns of the dimensions (0, 1) put one point into every elementary box 2^-a x 2^-(8 - a).  A
// mixed call takes its pad rows from erpl_design_value.  Prints one line per shape; exit status 1 on the first violation.
// Build with a host sanitizer through TABFLAGS (Makefile).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "erpl_qmc.h"

namespace {
struct Shape {
  int rows;
  int64_t n, block, first, count;
  int first_row;
};

const Shape kShapes[] = {{5, 64, 0, 0, 64, 0},     {7, 96, 32, 17, 50, 3},        {3, 1, 0, 0, 1, 0},
                         {4, 2147483647, 0, 1073754169, 64, 0}, {6, 4096, 512, 300, 1000, 1018}, {5, 300, 0, 0, 300, 314},
                         {11, 4097, 0, 1, 4095, 1015}};    // the last two rows of the last shape are pad rows

std::vector<uint32_t> V((size_t)ERPL_QMC_MAX_DIMS * ERPL_QMC_BITS);

int dim_of(int g) { return g < ERPL_QMC_MAX_DIMS ? g : -1; }

// global row g on dimension d (-1: a pad row under `pad`), columns [first, first + count) of the design, into out[count]
bool fill(uint64_t seed, int scramble, int pad, bool normal, const Shape& s, int g, int d, int64_t first, int64_t count, double* out) {
  const uint32_t m = (uint32_t)(s.block ? s.block : s.n), b = erpl_design_half_bits(m);
  bool capped = false;
  ErplDesignKeys K = {};
  uint32_t k0 = 0, k1 = 0;
  int64_t have = -1;
  for (int64_t c = 0; c < count; ++c) {
    const uint32_t i = (uint32_t)(first + c), rho = i / m, l = i - rho * m;
    if (have != (int64_t)rho) {
      erpl_qmc_keys(seed, (uint32_t)g, rho, &k0, &k1);
      K = erpl_design_keys(seed, (uint32_t)g, rho);
      have = rho;
    }
    out[c] = d >= 0 ? erpl_qmc_value(seed, scramble, normal, (uint32_t)g, i, V.data() + (size_t)d * ERPL_QMC_BITS, l, k0, k1)
                    : erpl_design_value(seed, pad, normal, (uint32_t)g, i, K.k, b, m, l, &capped);
  }
  return !capped;
}

int fail(const Shape& s, int r, const char* what) {
  printf("FAIL n=%lld block=%lld row=%d: %s\n", (long long)s.n, (long long)s.block, r, what);
  return 1;
}
}  // namespace

int main() {
  if (!erpl_qmc_expand(V.data())) { printf("FAIL: the table does not hold %d dimensions\n", ERPL_QMC_MAX_DIMS); return 1; }
  for (int d = 0; d < ERPL_QMC_MAX_DIMS; ++d)
    for (int j = 0; j < ERPL_QMC_BITS; ++j) {
      const uint32_t v = V[(size_t)d * ERPL_QMC_BITS + j], bit = (uint32_t)1 << (31 - j);
      if (!(v & bit) || (v & (bit - 1u))) { printf("FAIL: V[%d][%d] = %08x is not m 2^(31 - j) with an odd m\n", d, j, v); return 1; }
    }
  printf("ok table dims=%d\n", ERPL_QMC_MAX_DIMS);
  const uint64_t seed = 7;
  for (const Shape& s : kShapes) {
    const uint32_t m = (uint32_t)(s.block ? s.block : s.n);
    const bool whole = s.n <= 70000;
    std::vector<double> full((size_t)(whole ? s.n : 0)), win((size_t)s.count), z((size_t)s.count);
    std::vector<char> seen;
    for (int scramble = ERPL_QMC_RAW; scramble <= ERPL_QMC_OWEN; ++scramble)
      for (int r = 0; r < s.rows; ++r) {
        const int g = s.first_row + r, d = dim_of(g);
        if (!fill(seed, scramble, ERPL_DESIGN_LHS, false, s, g, d, s.first, s.count, win.data()) ||
            !fill(seed, scramble, ERPL_DESIGN_LHS, true, s, g, d, s.first, s.count, z.data()))
          return fail(s, r, "a cycle walk reached the cap");
        for (int64_t c = 0; c < s.count; ++c)
          if (!(win[(size_t)c] > 0.0 && win[(size_t)c] < 1.0) || !isfinite(z[(size_t)c])) return fail(s, r, "p outside (0, 1) or a normal value not finite");
        if (!whole) continue;
        if (!fill(seed, scramble, ERPL_DESIGN_LHS, false, s, g, d, 0, s.n, full.data())) return fail(s, r, "a cycle walk reached the cap");
        if (memcmp(win.data(), full.data() + s.first, (size_t)s.count * sizeof(double)) != 0) return fail(s, r, "the window differs from the full row");
        if (d < 0) continue;
        for (int64_t rep = 0; rep < s.n / m; ++rep)
          for (int k = 0; ((uint32_t)1 << k) <= m; ++k) {
            const uint32_t w = (uint32_t)1 << k;
            seen.assign(w, 0);
            for (uint32_t l = 0; l + w <= m; l += w) {
              memset(seen.data(), 0, w);
              for (uint32_t t = 0; t < w; ++t) {
                const uint32_t cell = (uint32_t)(full[(size_t)(rep * m + l + t)] * (double)w);   // exact: a power of two
                if (cell >= w || seen[cell]) return fail(s, r, "an aligned block of 2^k columns hits an interval twice");
                seen[cell] = 1;
              }
            }
          }
      }
    printf("ok rows=%d n=%lld block=%lld first=%lld count=%lld first_row=%d\n", s.rows, (long long)s.n, (long long)s.block,
           (long long)s.first, (long long)s.count, s.first_row);
  }
  // the pair (0, 1), 256 points, replicates 0 and 1 of block 256: one point per elementary box, seeds 0..7
  const Shape net = {2, 512, 256, 0, 512, 0};
  std::vector<double> x(512), y(512);
  for (uint64_t sd = 0; sd < 8; ++sd) {
    fill(sd, ERPL_QMC_OWEN, ERPL_DESIGN_RANDOM, false, net, 0, 0, 0, 512, x.data());
    fill(sd, ERPL_QMC_OWEN, ERPL_DESIGN_RANDOM, false, net, 1, 1, 0, 512, y.data());
    for (int rep = 0; rep < 2; ++rep)
      for (int a = 0; a <= 8; ++a) {
        char box[256] = {};
        for (int t = 0; t < 256; ++t) {
          const uint32_t bx = (uint32_t)(x[(size_t)(rep * 256 + t)] * (double)(1 << a)), by = (uint32_t)(y[(size_t)(rep * 256 + t)] * (double)(1 << (8 - a)));
          const uint32_t cell = (bx << (8 - a)) | by;
          if (cell >= 256 || box[cell]) return fail(net, a, "an elementary box of the pair (0, 1) is hit twice");
          box[cell] = 1;
        }
      }
  }
  printf("ok net pair=(0,1) points=256 replicates=2 seeds=8\n");
  return 0;
}
