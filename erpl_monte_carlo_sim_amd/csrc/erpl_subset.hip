// erpl_subset.hip — erpl_mc_subset_* of the C ABI (include/erpl_mc.h): the five steps of a level of subset simulation.  The
// rule is erpl_subset.h, here for the device (the kernels below) and for the host (the _host calls); built without FMA
// contraction, so that rho x + s xi and x + w (u - 0.5) round alike on both.
//
// What binds each kernel (DESIGN.md section 8.15 has the measurements, or says UNMEASURED):
//   subset_propose      vector issue: Philox (about 100 integer ops) and PPND16 (two degree-7 Horner chains, a log, a sqrt, a
//                       divide, all fp64) per 16 bytes moved - an erpl_design_fill with one more load
//   subset_gather       HBM bytes: permuted 8-byte reads (a whole 64-byte sector per element where the seeds are sparse),
//                       coalesced writes
//   subset_commit       HBM bytes: one coalesced read (the chosen source) and one write per element
//   subset_limit_state  HBM bytes, 3 to 5 rows of the summary in and one out
//   the selection       eight passes over g (8 bytes per sample each) plus three for the compaction: launch-bound below
//                       some 10^6 samples
//   subset_chain_stats  L2: steps^2 / 2 byte reads per chain out of a steps * chains byte array
#include "erpl_host.h"

#include "erpl_stat_device.h"
#include "erpl_subset.h"

namespace {
constexpr int kBlock = ERPL_ANA_BLOCK;          // 256: the folds of erpl_stat_device.h are written for it
constexpr int kTileIters = 8;
constexpr int kTile = kBlock * kTileIters;      // columns of a workgroup of the compaction
constexpr int kCommitRows = 8;                  // rows of a workgroup of the commit

// the device workspace: this block, then the rows' parameters, then the (before, equal) counts of the compaction's tiles
struct SubsetState {
  u64 prefix, rank, alive;
  u64 hist[ERPL_ANA_BINS];
};
constexpr size_t kParamsAt = 4096;
constexpr size_t kParamsBytes = (size_t)ERPL_DESIGN_MAX_ROWS * (3 * sizeof(double) + 1);
constexpr size_t kTilesAt = kParamsAt + ((kParamsBytes + 255) / 256) * 256;
static_assert(sizeof(SubsetState) <= kParamsAt, "the selection state fits its slot");

// ---------------------------------------------------------------- the limit state

__global__ __launch_bounds__(kBlock) void subset_limit_state(const erpl_subset_spec s, const double* __restrict__ summary,
                                                             const int32_t* __restrict__ status, int64_t ld, int64_t n,
                                                             double* __restrict__ g) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double v[ERPL_SUMMARY_DIM];
#pragma unroll
  for (int r = 0; r < ERPL_SUMMARY_DIM; ++r) v[r] = 0.0;
  v[ERPL_SUM_APOGEE_ALT] = summary[(int64_t)ERPL_SUM_APOGEE_ALT * ld + i];
  v[ERPL_SUM_RANGE] = summary[(int64_t)ERPL_SUM_RANGE * ld + i];
  v[ERPL_SUM_FLIGHT_TIME] = summary[(int64_t)ERPL_SUM_FLIGHT_TIME * ld + i];
  if (s.use_centre) {
    v[ERPL_SUM_IMPACT_X] = summary[(int64_t)ERPL_SUM_IMPACT_X * ld + i];
    v[ERPL_SUM_IMPACT_Y] = summary[(int64_t)ERPL_SUM_IMPACT_Y * ld + i];
  } else {
    const double x = summary[(int64_t)s.row * ld + i];   // s.row is the workgroup's: one more uniform row
#pragma unroll
    for (int r = 0; r < ERPL_SUMMARY_DIM; ++r)
      if (r == s.row) v[r] = x;
  }
  g[i] = erpl_subset_g(s, v, status != nullptr, status ? status[i] : 0);
}

// ---------------------------------------------------------------- the selection of the n_seeds-th key

// One digit of the radix selection of erpl_stat_device.h (select_count, select_scan): the histogram of the digit at `shift`
// over the keys that match the prefix above it, in LDS, then one 64-bit integer add per bin and workgroup.
__global__ __launch_bounds__(kBlock) void subset_hist(const double* __restrict__ g, int64_t n, int shift, SubsetState* st) {
  __shared__ unsigned int hist[1][ERPL_ANA_BINS];
  hist[0][threadIdx.x] = 0u;
  __syncthreads();
  const int lead = 0;
  const u64 prefix = st->prefix;      // written by the launch before: uniform
  u64 alive = 0ull;
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    const bool use = i < n;
    const double v = use ? g[i] : 0.0;
    select_count(hist, &lead, &prefix, 1, use, erpl_subset_key(v), shift, 1u);
    if (shift == 56) alive += (u64)__popcll(__ballot(use && erpl_subset_alive(v)));
  }
  __syncthreads();
  const unsigned int h = hist[0][threadIdx.x];
  if (h) atomicAdd(&st->hist[threadIdx.x], (u64)h);
  if (shift == 56 && (threadIdx.x & 63) == 0 && alive) atomicAdd(&st->alive, alive);
}

// the state of a selection: nothing counted, no digit decided, the rank of the n_seeds-th sample
__global__ __launch_bounds__(kBlock) void subset_init(SubsetState* st, u64 rank) {
  st->hist[threadIdx.x] = 0ull;
  if (threadIdx.x == 0) { st->prefix = 0ull; st->rank = rank; st->alive = 0ull; }
}

// One wave: the bin that holds the rank, into the prefix; the histogram cleared for the next pass.  After the last digit the
// prefix is the key of the n_seeds-th sample and the rank its place among the samples of that key.
__global__ __launch_bounds__(64) void subset_pick(SubsetState* st, int shift, double* threshold, int64_t* n_alive) {
  const int lane = threadIdx.x;
  int digit = 0;
  u64 below = 0ull;
  const bool mine = select_scan(st->hist, st->rank, lane, &digit, &below);
  __syncthreads();
  if (mine) {
    st->prefix |= (u64)digit << shift;
    st->rank -= below;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) st->hist[lane * 4 + k] = 0ull;
  __syncthreads();
  if (shift == 0 && lane == 0) {
    *threshold = erpl_subset_g_of_key(st->prefix);
    *n_alive = (int64_t)st->alive;
  }
}

// ---------------------------------------------------------------- the stable compaction

// per tile of kTile columns: the keys before the threshold key and the keys equal to it
__global__ __launch_bounds__(kBlock) void subset_tile_counts(const double* __restrict__ g, int64_t n, const SubsetState* st,
                                                             u64* __restrict__ tiles) {
  const u64 key = st->prefix;
  u64 cnt[2] = {0ull, 0ull};
  const int64_t base = (int64_t)blockIdx.x * kTile;
  for (int it = 0; it < kTileIters; ++it) {
    const int64_t i = base + (int64_t)it * kBlock + threadIdx.x;
    const bool use = i < n;
    const u64 k = erpl_subset_key(use ? g[i] : 0.0);
    cnt[0] += (u64)__popcll(__ballot(use && k < key));
    cnt[1] += (u64)__popcll(__ballot(use && k == key));
  }
  const u64 total = counters_fold<2>(cnt);
  if (threadIdx.x < 2) tiles[2 * (size_t)blockIdx.x + threadIdx.x] = total;
}

// one workgroup: the tiles' counts become exclusive prefix sums, in place
__global__ __launch_bounds__(kBlock) void subset_tile_scan(u64* __restrict__ tiles, int64_t n_tiles) {
  __shared__ u64 s_wave[kWaves][2];
  __shared__ u64 s_carry[2];
  if (threadIdx.x < 2) s_carry[threadIdx.x] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = 0; base < n_tiles; base += kBlock) {
    const int64_t t = base + threadIdx.x;
    const u64 a = t < n_tiles ? tiles[2 * t] : 0ull, b = t < n_tiles ? tiles[2 * t + 1] : 0ull;
    u64 ia = a, ib = b;
    for (int off = 1; off < 64; off <<= 1) {
      const u64 ua = __shfl_up(ia, off), ub = __shfl_up(ib, off);
      if (lane >= off) { ia += ua; ib += ub; }
    }
    if (lane == 63) { s_wave[wave][0] = ia; s_wave[wave][1] = ib; }
    __syncthreads();
    u64 oa = s_carry[0], ob = s_carry[1];
    for (int w = 0; w < wave; ++w) { oa += s_wave[w][0]; ob += s_wave[w][1]; }
    if (t < n_tiles) { tiles[2 * t] = oa + ia - a; tiles[2 * t + 1] = ob + ib - b; }
    __syncthreads();
    if (threadIdx.x == kBlock - 1) { s_carry[0] = oa + ia; s_carry[1] = ob + ib; }
    __syncthreads();
  }
}

// selected[i] and the place of every selected sample among them, ascending in id: the keys before the threshold key all,
// of the keys equal to it the first rank + 1 in id order (ballots within a wave, a scan over the waves, the tile's offset)
__global__ __launch_bounds__(kBlock) void subset_tile_write(const double* __restrict__ g, int64_t n, int64_t n_seeds,
                                                            const SubsetState* st, const u64* __restrict__ tiles,
                                                            int32_t* __restrict__ idx, uint8_t* __restrict__ selected) {
  __shared__ u64 s_wave[kWaves][2];
  const u64 key = st->prefix, need = st->rank + 1ull;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 lower = lane ? (~0ull >> (64 - lane)) : 0ull;   // the lanes below this one
  u64 run_lt = tiles[2 * (size_t)blockIdx.x], run_eq = tiles[2 * (size_t)blockIdx.x + 1];
  const int64_t base = (int64_t)blockIdx.x * kTile;
  for (int it = 0; it < kTileIters; ++it) {
    const int64_t i = base + (int64_t)it * kBlock + threadIdx.x;
    const bool use = i < n;
    const u64 k = erpl_subset_key(use ? g[i] : 0.0);
    const bool lt = use && k < key, eq = use && k == key;
    const u64 m_lt = __ballot(lt), m_eq = __ballot(eq);
    if (lane == 0) { s_wave[wave][0] = (u64)__popcll(m_lt); s_wave[wave][1] = (u64)__popcll(m_eq); }
    __syncthreads();
    u64 lt_before = run_lt, eq_before = run_eq, all_lt = 0ull, all_eq = 0ull;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) { lt_before += s_wave[w][0]; eq_before += s_wave[w][1]; }
      all_lt += s_wave[w][0]; all_eq += s_wave[w][1];
    }
    lt_before += (u64)__popcll(m_lt & lower);
    eq_before += (u64)__popcll(m_eq & lower);
    const bool sel = lt || (eq && eq_before < need);
    if (use) selected[i] = sel ? 1 : 0;
    if (sel) {
      const u64 at = lt_before + (eq_before < need ? eq_before : need);
      if (at < (u64)n_seeds) idx[at] = (int32_t)i;   // always, unless the counts were wrong: never a store past idx
    }
    run_lt += all_lt; run_eq += all_eq;
    __syncthreads();
  }
}

// dst[r][k] = src[r][idx[k]]: blockIdx.y the row, k fastest - permuted reads, coalesced writes
template <class E>
__global__ __launch_bounds__(kBlock) void subset_gather(const E* __restrict__ src, int64_t ld_src, E* __restrict__ dst,
                                                        int64_t ld_dst, const int32_t* __restrict__ idx, int64_t n_seeds, int64_t n) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n_seeds) return;
  const int64_t j = idx[k];
  if (j < 0 || j >= n) return;
  dst[(int64_t)blockIdx.y * ld_dst + k] = src[(int64_t)blockIdx.y * ld_src + j];
}

// n_seeds = 0: the indicator of a given threshold and its count (ballots, one integer atomic per workgroup)
__global__ __launch_bounds__(kBlock) void subset_indicator(const double* __restrict__ g, int64_t n, const double* __restrict__ threshold,
                                                           uint8_t* __restrict__ selected, u64* count) {
  const double b = *threshold;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool in = i < n && g[i] >= b;
  if (i < n) selected[i] = in ? 1 : 0;
  u64 cnt[1] = {(u64)__popcll(__ballot(in))};
  const u64 total = counters_fold<1>(cnt);
  if (threadIdx.x == 0 && total) atomicAdd(count, total);
}

// ---------------------------------------------------------------- the proposal

// One thread per (row, chain), chains fastest: a wave loads and stores 512 contiguous bytes.  blockIdx.y is the row, so kind,
// rho, s and w are the workgroup's own (uniform loads).
__global__ __launch_bounds__(kBlock) void subset_propose(const uint64_t seed, const uint32_t level, const uint32_t step,
                                                         const double* __restrict__ rho, const double* __restrict__ s,
                                                         const double* __restrict__ w, const uint8_t* __restrict__ kinds,
                                                         const double* __restrict__ cur, int64_t ld, uint32_t first_chain,
                                                         int64_t count, double* __restrict__ cand, int64_t ld_cand) {
  const uint32_t row = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= count) return;
  cand[(int64_t)row * ld_cand + c] = erpl_subset_candidate(kinds[row] == ERPL_DESIGN_NORMAL, cur[(int64_t)row * ld + c], rho[row],
                                                           s[row], w[row], seed, level, step, row, first_chain + (uint32_t)c);
}

// ---------------------------------------------------------------- the commit

struct CommitArgs {
  erpl_subset_triple t[ERPL_SUBSET_MAX_SLOTS];
  int32_t first[ERPL_SUBSET_MAX_SLOTS + 1];   // triple q owns the rows first[q] .. first[q + 1] - 1 of the call
  int32_t n_triples;
};

template <class E>
__device__ __forceinline__ void commit_row(const erpl_subset_triple& t, int r, int64_t c, bool take) {
  const E* from = take ? (const E*)t.cand + (int64_t)r * t.ld_cand : (const E*)t.cur + (int64_t)r * t.ld;
  ((E*)t.next)[(int64_t)r * t.ld + c] = from[c];
}

// One thread per column and kCommitRows rows of the call (blockIdx.y), columns fastest.  A thread reads its column's decision
// once; the workgroups of blockIdx.y == 0 also write g_next and count the accepted.
__global__ __launch_bounds__(kBlock) void subset_commit(const CommitArgs a, const double* __restrict__ threshold,
                                                        const double* __restrict__ g_cand, const double* __restrict__ g_cur,
                                                        double* __restrict__ g_next, int64_t count, u64* n_accepted) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool use = c < count;
  const double gc = use ? g_cand[c] : 0.0;
  const bool take = use && gc >= *threshold;
  if (blockIdx.y == 0) {
    if (use) g_next[c] = take ? gc : g_cur[c];
    u64 cnt[1] = {(u64)__popcll(__ballot(take))};
    const u64 total = counters_fold<1>(cnt);
    if (threadIdx.x == 0 && total) atomicAdd(n_accepted, total);
  }
  if (!use) return;
  const int r0 = (int)blockIdx.y * kCommitRows;
  for (int k = 0; k < kCommitRows; ++k) {
    const int r = r0 + k;
    if (r >= a.first[a.n_triples]) return;
    int q = 0;
    while (q + 1 < a.n_triples && r >= a.first[q + 1]) ++q;   // at most 3 trips
    const erpl_subset_triple& t = a.t[q];
    if (t.elem_size == 8) commit_row<uint64_t>(t, r - a.first[q], c, take);
    else if (t.elem_size == 4) commit_row<uint32_t>(t, r - a.first[q], c, take);
    else commit_row<uint8_t>(t, r - a.first[q], c, take);
  }
}

// ---------------------------------------------------------------- the chain statistics

// blockIdx.y = k: 0 counts the ones, k >= 1 the pairs at lag k; one thread per chain, ballots, one integer atomic per workgroup
__global__ __launch_bounds__(kBlock) void subset_chain_stats(const uint8_t* __restrict__ sel, int64_t C, int64_t T, u64* n1, u64* pair) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t k = blockIdx.y;
  const bool use = j < C;
  u64 sum = 0ull;
  if (use)
    for (int64_t t = 0; t + k < T; ++t) sum += (sel[t * C + j] && sel[(t + k) * C + j]) ? 1ull : 0ull;
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
  u64 cnt[1] = {(u64)__shfl(sum, 0)};
  const u64 total = counters_fold<1>(cnt);
  if (threadIdx.x == 0 && total) atomicAdd(k == 0 ? n1 : pair + (k - 1), total);
}

// ---------------------------------------------------------------- the refusals, in the order of the header

bool unit(double v) { return v >= 0.0 && v <= 1.0; }
bool elem_ok(int e) { return e == 1 || e == 4 || e == 8; }
constexpr int64_t kMostColumns = ((int64_t)1 << 31) - 1;

int limit_state_check(const erpl_subset_spec* s, const double* summary, int64_t ld, int64_t n, const double* g) {
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (!summary) return erpl_fail(ERPL_ERR_INVALID, "summary is NULL");
  if (!g) return erpl_fail(ERPL_ERR_INVALID, "g is NULL");
  const double bound[5] = {s->max_apogee, s->min_apogee, s->max_range, s->max_flight_time, s->energy_apogee};
  for (int b = 0; b < 5; ++b)
    if (bound[b] != bound[b]) return erpl_fail(ERPL_ERR_INVALID, "bound %d of the filter is NaN", b);
  if (s->row < 0 || s->row >= ERPL_SUMMARY_DIM) return erpl_fail(ERPL_ERR_INVALID, "row = %d outside 0..15", s->row);
  if (s->sign != 1 && s->sign != -1) return erpl_fail(ERPL_ERR_INVALID, "sign = %d is neither +1 nor -1", s->sign);
  if (s->use_centre && !(erpl_is_finite(s->cx) && erpl_is_finite(s->cy))) return erpl_fail(ERPL_ERR_INVALID, "the centre (cx, cy) is not finite");
  if (n < 1 || n > kMostColumns) return erpl_fail(ERPL_ERR_INVALID, "n = %lld outside 1 .. 2^31 - 1", (long long)n);
  if (ld < n) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below n = %lld", (long long)ld, (long long)n);
  return ERPL_OK;
}

int seeds_check(const double* g, int64_t n, int64_t n_seeds, const int32_t* idx, const uint8_t* selected, const double* threshold,
                const int64_t* n_alive, const erpl_subset_gather* gathers, int32_t n_gathers) {
  if (!g) return erpl_fail(ERPL_ERR_INVALID, "g is NULL");
  if (!selected) return erpl_fail(ERPL_ERR_INVALID, "selected is NULL");
  if (!threshold) return erpl_fail(ERPL_ERR_INVALID, "threshold is NULL");
  if (!n_alive) return erpl_fail(ERPL_ERR_INVALID, "n_alive is NULL");
  if (n < 1 || n > kMostColumns) return erpl_fail(ERPL_ERR_INVALID, "n = %lld outside 1 .. 2^31 - 1", (long long)n);
  if (n_seeds < 0 || n_seeds > n) return erpl_fail(ERPL_ERR_INVALID, "n_seeds = %lld outside 0 .. n = %lld", (long long)n_seeds, (long long)n);
  if (n_seeds > 0 && !idx) return erpl_fail(ERPL_ERR_INVALID, "idx is NULL");
  if (n_gathers < 0 || n_gathers > ERPL_SUBSET_MAX_SLOTS || (n_gathers > 0 && n_seeds == 0))
    return erpl_fail(ERPL_ERR_INVALID, "n_gathers = %d outside 0 .. %d, or above 0 with n_seeds = 0", n_gathers, ERPL_SUBSET_MAX_SLOTS);
  if (n_gathers > 0 && !gathers) return erpl_fail(ERPL_ERR_INVALID, "gathers is NULL");
  for (int q = 0; q < n_gathers; ++q) {
    const erpl_subset_gather& t = gathers[q];
    if (!t.src) return erpl_fail(ERPL_ERR_INVALID, "gathers[%d].src is NULL", q);
    if (!t.dst) return erpl_fail(ERPL_ERR_INVALID, "gathers[%d].dst is NULL", q);
    if (t.rows < 1 || t.rows > ERPL_DESIGN_MAX_ROWS) return erpl_fail(ERPL_ERR_INVALID, "gathers[%d].rows = %d outside 1 .. %d", q, t.rows, ERPL_DESIGN_MAX_ROWS);
    if (!elem_ok(t.elem_size)) return erpl_fail(ERPL_ERR_INVALID, "gathers[%d].elem_size = %d is not 1, 4 or 8", q, t.elem_size);
    if (t.ld_src < n) return erpl_fail(ERPL_ERR_INVALID, "gathers[%d].ld_src = %lld is below n = %lld", q, (long long)t.ld_src, (long long)n);
    if (t.ld_dst < n_seeds) return erpl_fail(ERPL_ERR_INVALID, "gathers[%d].ld_dst = %lld is below n_seeds = %lld", q, (long long)t.ld_dst, (long long)n_seeds);
  }
  return ERPL_OK;
}

int propose_check(const erpl_subset_spec* sp, const uint8_t* kinds, const double* rho, const double* s, const double* w, int32_t rows,
                  const double* cur, int64_t ld, int64_t first_chain, int64_t count, const double* cand, int64_t ld_cand) {
  if (!sp) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (!kinds) return erpl_fail(ERPL_ERR_INVALID, "kinds is NULL");
  if (!rho) return erpl_fail(ERPL_ERR_INVALID, "rho is NULL");
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "s is NULL");
  if (!w) return erpl_fail(ERPL_ERR_INVALID, "w is NULL");
  if (!cur) return erpl_fail(ERPL_ERR_INVALID, "cur is NULL");
  if (!cand) return erpl_fail(ERPL_ERR_INVALID, "cand is NULL");
  if (rows < 1 || rows > ERPL_DESIGN_MAX_ROWS) return erpl_fail(ERPL_ERR_INVALID, "rows = %d outside 1 .. %d", rows, ERPL_DESIGN_MAX_ROWS);
  if (sp->step > ERPL_SUBSET_MAX_STEPS) return erpl_fail(ERPL_ERR_INVALID, "step = %u exceeds %d", sp->step, ERPL_SUBSET_MAX_STEPS);
  if (first_chain < 0) return erpl_fail(ERPL_ERR_INVALID, "first_chain = %lld is negative", (long long)first_chain);
  if (count < 0) return erpl_fail(ERPL_ERR_INVALID, "count = %lld is negative", (long long)count);
  if (first_chain > kMostColumns || count > kMostColumns - first_chain)
    return erpl_fail(ERPL_ERR_INVALID, "first_chain + count = %lld + %lld exceeds 2^31 - 1", (long long)first_chain, (long long)count);
  if (ld < count) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below count = %lld", (long long)ld, (long long)count);
  if (ld_cand < count) return erpl_fail(ERPL_ERR_INVALID, "ld_cand = %lld is below count = %lld", (long long)ld_cand, (long long)count);
  for (int32_t r = 0; r < rows; ++r) {
    if (kinds[r] != ERPL_DESIGN_UNIFORM && kinds[r] != ERPL_DESIGN_NORMAL)
      return erpl_fail(ERPL_ERR_INVALID, "kinds[%d] = %d is neither ERPL_DESIGN_UNIFORM nor ERPL_DESIGN_NORMAL", r, (int)kinds[r]);
    if (!unit(rho[r])) return erpl_fail(ERPL_ERR_INVALID, "rho[%d] = %g outside [0, 1]", r, rho[r]);
    if (!unit(s[r])) return erpl_fail(ERPL_ERR_INVALID, "s[%d] = %g outside [0, 1]", r, s[r]);
    if (!unit(w[r])) return erpl_fail(ERPL_ERR_INVALID, "w[%d] = %g outside [0, 1]", r, w[r]);
  }
  return ERPL_OK;
}

int commit_check(const double* threshold, const double* g_cand, const double* g_cur, const double* g_next, const erpl_subset_triple* triples,
                 int32_t n_triples, int64_t count, const int64_t* n_accepted) {
  if (!threshold) return erpl_fail(ERPL_ERR_INVALID, "threshold is NULL");
  if (!g_cand) return erpl_fail(ERPL_ERR_INVALID, "g_cand is NULL");
  if (!g_cur) return erpl_fail(ERPL_ERR_INVALID, "g_cur is NULL");
  if (!g_next) return erpl_fail(ERPL_ERR_INVALID, "g_next is NULL");
  if (!n_accepted) return erpl_fail(ERPL_ERR_INVALID, "n_accepted is NULL");
  if (n_triples < 0 || n_triples > ERPL_SUBSET_MAX_SLOTS) return erpl_fail(ERPL_ERR_INVALID, "n_triples = %d outside 0 .. %d", n_triples, ERPL_SUBSET_MAX_SLOTS);
  if (n_triples > 0 && !triples) return erpl_fail(ERPL_ERR_INVALID, "triples is NULL");
  for (int q = 0; q < n_triples; ++q) {
    const erpl_subset_triple& t = triples[q];
    if (!t.cand) return erpl_fail(ERPL_ERR_INVALID, "triples[%d].cand is NULL", q);
    if (!t.cur) return erpl_fail(ERPL_ERR_INVALID, "triples[%d].cur is NULL", q);
    if (!t.next) return erpl_fail(ERPL_ERR_INVALID, "triples[%d].next is NULL", q);
    if (t.rows < 1 || t.rows > ERPL_DESIGN_MAX_ROWS) return erpl_fail(ERPL_ERR_INVALID, "triples[%d].rows = %d outside 1 .. %d", q, t.rows, ERPL_DESIGN_MAX_ROWS);
    if (!elem_ok(t.elem_size)) return erpl_fail(ERPL_ERR_INVALID, "triples[%d].elem_size = %d is not 1, 4 or 8", q, t.elem_size);
    if (t.ld_cand < count) return erpl_fail(ERPL_ERR_INVALID, "triples[%d].ld_cand = %lld is below count = %lld", q, (long long)t.ld_cand, (long long)count);
    if (t.ld < count) return erpl_fail(ERPL_ERR_INVALID, "triples[%d].ld = %lld is below count = %lld", q, (long long)t.ld, (long long)count);
  }
  if (count < 0) return erpl_fail(ERPL_ERR_INVALID, "count = %lld is negative", (long long)count);
  return ERPL_OK;
}

int chain_stats_check(const uint8_t* selected, int64_t C, int64_t T, const int64_t* n1, const int64_t* pair) {
  if (!selected) return erpl_fail(ERPL_ERR_INVALID, "selected is NULL");
  if (!n1) return erpl_fail(ERPL_ERR_INVALID, "n1 is NULL");
  if (C < 1) return erpl_fail(ERPL_ERR_INVALID, "chains = %lld is below 1", (long long)C);
  if (T < 1 || T > ERPL_SUBSET_MAX_STEPS) return erpl_fail(ERPL_ERR_INVALID, "steps = %lld outside 1 .. %d", (long long)T, ERPL_SUBSET_MAX_STEPS);
  if (C > kMostColumns / T) return erpl_fail(ERPL_ERR_INVALID, "chains * steps = %lld * %lld exceeds 2^31 - 1", (long long)C, (long long)T);
  if (T > 1 && !pair) return erpl_fail(ERPL_ERR_INVALID, "pair is NULL");
  return ERPL_OK;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// the context's workspace with room for the tiles of n columns
int workspace(erpl_ctx* c, int64_t n, char** base) {
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n_tiles = (n + kTile - 1) / kTile;
  ERPL_TRY(c->subset.grow(kTilesAt + (size_t)n_tiles * 2 * sizeof(u64)));
  *base = c->subset.buf;
  return ERPL_OK;
}
}  // namespace

extern "C" {

int erpl_mc_subset_defaults(erpl_subset_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  *spec = erpl_subset_spec{};
  erpl_analysis_spec a;
  ERPL_TRY(erpl_mc_analysis_defaults(&a));
  spec->max_apogee = a.max_apogee; spec->min_apogee = a.min_apogee; spec->max_range = a.max_range;
  spec->max_flight_time = a.max_flight_time; spec->energy_apogee = a.energy_apogee;
  spec->row = ERPL_SUM_RANGE;
  spec->sign = 1;
  spec->step = 1;
  return ERPL_OK;
}

int erpl_mc_subset_limit_state(erpl_ctx* c, const erpl_subset_spec* spec, const double* summary, const int32_t* status, int64_t ld,
                               int64_t n, double* g, void* stream) {
  ERPL_TRY(limit_state_check(spec, summary, ld, n, g));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(subset_limit_state, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)stream, *spec, summary, status, ld, n, g);
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

int erpl_mc_subset_limit_state_host(const erpl_subset_spec* spec, const double* summary, const int32_t* status, int64_t ld, int64_t n,
                                    double* g) {
  ERPL_TRY(limit_state_check(spec, summary, ld, n, g));
  for (int64_t i = 0; i < n; ++i) {
    double v[ERPL_SUMMARY_DIM];
    for (int r = 0; r < ERPL_SUMMARY_DIM; ++r) v[r] = summary[(int64_t)r * ld + i];
    g[i] = erpl_subset_g(*spec, v, status != nullptr, status ? status[i] : 0);
  }
  return ERPL_OK;
}

int erpl_mc_subset_seeds(erpl_ctx* c, const double* g, int64_t n, int64_t n_seeds, int32_t* idx, uint8_t* selected, double* threshold,
                         int64_t* n_alive, const erpl_subset_gather* gathers, int32_t n_gathers, void* stream) {
  ERPL_TRY(seeds_check(g, n, n_seeds, idx, selected, threshold, n_alive, gathers, n_gathers));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  char* base = nullptr;
  ERPL_TRY(workspace(c, n, &base));
  hipStream_t st = (hipStream_t)stream;
  if (n_seeds == 0) {
    HIP_TRY(hipMemsetAsync(n_alive, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(subset_indicator, dim3(blocks_of(n)), dim3(kBlock), 0, st, g, n, (const double*)threshold, selected, (u64*)n_alive);
    HIP_TRY(hipGetLastError());
    return ERPL_OK;
  }
  SubsetState* state = (SubsetState*)base;
  u64* tiles = (u64*)(base + kTilesAt);
  const int64_t n_tiles = (n + kTile - 1) / kTile;
  hipLaunchKernelGGL(subset_init, dim3(1), dim3(kBlock), 0, st, state, (u64)(n_seeds - 1));
  for (int shift = 56; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(subset_hist, dim3((unsigned)grid_of(n)), dim3(kBlock), 0, st, g, n, shift, state);
    hipLaunchKernelGGL(subset_pick, dim3(1), dim3(64), 0, st, state, shift, threshold, n_alive);
  }
  hipLaunchKernelGGL(subset_tile_counts, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, g, n, (const SubsetState*)state, tiles);
  hipLaunchKernelGGL(subset_tile_scan, dim3(1), dim3(kBlock), 0, st, tiles, n_tiles);
  hipLaunchKernelGGL(subset_tile_write, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, g, n, n_seeds, (const SubsetState*)state,
                     (const u64*)tiles, idx, selected);
  for (int q = 0; q < n_gathers; ++q) {
    const erpl_subset_gather& t = gathers[q];
    const dim3 grid(blocks_of(n_seeds), (unsigned)t.rows);
    if (t.elem_size == 8)
      hipLaunchKernelGGL(subset_gather<uint64_t>, grid, dim3(kBlock), 0, st, (const uint64_t*)t.src, t.ld_src, (uint64_t*)t.dst, t.ld_dst,
                         (const int32_t*)idx, n_seeds, n);
    else if (t.elem_size == 4)
      hipLaunchKernelGGL(subset_gather<uint32_t>, grid, dim3(kBlock), 0, st, (const uint32_t*)t.src, t.ld_src, (uint32_t*)t.dst, t.ld_dst,
                         (const int32_t*)idx, n_seeds, n);
    else
      hipLaunchKernelGGL(subset_gather<uint8_t>, grid, dim3(kBlock), 0, st, (const uint8_t*)t.src, t.ld_src, (uint8_t*)t.dst, t.ld_dst,
                         (const int32_t*)idx, n_seeds, n);
  }
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

int erpl_mc_subset_seeds_host(const double* g, int64_t n, int64_t n_seeds, int32_t* idx, uint8_t* selected, double* threshold,
                              int64_t* n_alive, const erpl_subset_gather* gathers, int32_t n_gathers) {
  ERPL_TRY(seeds_check(g, n, n_seeds, idx, selected, threshold, n_alive, gathers, n_gathers));
  if (!erpl_subset_seeds_rule(g, n, n_seeds, idx, selected, threshold, n_alive, gathers, n_gathers))
    return erpl_fail(ERPL_ERR_INVALID, "the level has died out: %lld samples with g > -inf, n_seeds = %lld", (long long)*n_alive,
                     (long long)n_seeds);
  return ERPL_OK;
}

int erpl_mc_subset_propose(erpl_ctx* c, const erpl_subset_spec* spec, const uint8_t* kinds, const double* rho, const double* s,
                           const double* w, int32_t rows, const double* cur, int64_t ld, int64_t first_chain, int64_t count, double* cand,
                           int64_t ld_cand, void* stream) {
  ERPL_TRY(propose_check(spec, kinds, rho, s, w, rows, cur, ld, first_chain, count, cand, ld_cand));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (count == 0) return ERPL_OK;
  char* base = nullptr;
  ERPL_TRY(workspace(c, 1, &base));
  hipStream_t st = (hipStream_t)stream;
  // the rows' parameters go up through the context's pinned staging: rho, s, w, then the kinds.  The staging is written
  // again only once the copy of the call before has left it (an event; that copy sits behind nothing but earlier subset work)
  if (!c->subset_pin) {
    HIP_TRY(hipHostMalloc((void**)&c->subset_pin, kParamsBytes, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&c->subset_ev, hipEventDisableTiming));
  } else {
    HIP_TRY(hipEventSynchronize(c->subset_ev));
  }
  const size_t row_bytes = (size_t)rows * sizeof(double);
  memcpy(c->subset_pin, rho, row_bytes);
  memcpy(c->subset_pin + row_bytes, s, row_bytes);
  memcpy(c->subset_pin + 2 * row_bytes, w, row_bytes);
  memcpy(c->subset_pin + 3 * row_bytes, kinds, (size_t)rows);
  HIP_TRY(hipMemcpyAsync(base + kParamsAt, c->subset_pin, 3 * row_bytes + (size_t)rows, hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(c->subset_ev, st));
  const double* d_rho = (const double*)(base + kParamsAt);
  const double *d_s = d_rho + rows, *d_w = d_s + rows;
  const uint8_t* d_kinds = (const uint8_t*)(d_w + rows);
  hipLaunchKernelGGL(subset_propose, dim3(blocks_of(count), (unsigned)rows), dim3(kBlock), 0, st, spec->seed, spec->level, spec->step,
                     d_rho, d_s, d_w, d_kinds, cur, ld, (uint32_t)first_chain,
                     count, cand, ld_cand);
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

int erpl_mc_subset_propose_host(const erpl_subset_spec* spec, const uint8_t* kinds, const double* rho, const double* s, const double* w,
                                int32_t rows, const double* cur, int64_t ld, int64_t first_chain, int64_t count, double* cand,
                                int64_t ld_cand) {
  ERPL_TRY(propose_check(spec, kinds, rho, s, w, rows, cur, ld, first_chain, count, cand, ld_cand));
  erpl_subset_propose_rule(*spec, kinds, rho, s, w, rows, cur, ld, first_chain, count, cand, ld_cand);
  return ERPL_OK;
}

int erpl_mc_subset_commit(erpl_ctx* c, const double* threshold, const double* g_cand, const double* g_cur, double* g_next,
                          const erpl_subset_triple* triples, int32_t n_triples, int64_t count, int64_t* n_accepted, void* stream) {
  ERPL_TRY(commit_check(threshold, g_cand, g_cur, g_next, triples, n_triples, count, n_accepted));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (count == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  CommitArgs a = {};
  a.n_triples = n_triples;
  for (int q = 0; q < n_triples; ++q) {
    a.t[q] = triples[q];
    a.first[q + 1] = a.first[q] + triples[q].rows;
  }
  const int total = a.first[n_triples];
  const unsigned gy = (unsigned)((total + kCommitRows - 1) / kCommitRows);
  hipLaunchKernelGGL(subset_commit, dim3(blocks_of(count), gy ? gy : 1u), dim3(kBlock), 0, (hipStream_t)stream, a, threshold, g_cand, g_cur,
                     g_next, count, (u64*)n_accepted);
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

int erpl_mc_subset_commit_host(const double* threshold, const double* g_cand, const double* g_cur, double* g_next,
                               const erpl_subset_triple* triples, int32_t n_triples, int64_t count, int64_t* n_accepted) {
  ERPL_TRY(commit_check(threshold, g_cand, g_cur, g_next, triples, n_triples, count, n_accepted));
  erpl_subset_commit_rule(*threshold, g_cand, g_cur, g_next, triples, n_triples, count, n_accepted);
  return ERPL_OK;
}

int erpl_mc_subset_chain_stats(erpl_ctx* c, const uint8_t* selected, int64_t C, int64_t T, int64_t* n1, int64_t* pair, void* stream) {
  ERPL_TRY(chain_stats_check(selected, C, T, n1, pair));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(n1, 0, sizeof(int64_t), st));
  if (T > 1) HIP_TRY(hipMemsetAsync(pair, 0, (size_t)(T - 1) * sizeof(int64_t), st));
  hipLaunchKernelGGL(subset_chain_stats, dim3(blocks_of(C), (unsigned)T), dim3(kBlock), 0, st, selected, C, T, (u64*)n1, (u64*)pair);
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

int erpl_mc_subset_chain_stats_host(const uint8_t* selected, int64_t C, int64_t T, int64_t* n1, int64_t* pair) {
  ERPL_TRY(chain_stats_check(selected, C, T, n1, pair));
  erpl_subset_chain_stats_rule(selected, C, T, n1, pair);
  return ERPL_OK;
}

}  // extern "C"
