// erpl_tally.hip — erpl_mc_tally_* of the C ABI (include/erpl_mc.h): a run of any length folded into a fixed-size state of
// int64 words.  What a sample contributes is erpl_tally.h, here for the device (the kernels below) and for the host
// (erpl_mc_tally_*_host); built without FMA contraction, the one FMA of the rule (lo = fma(d, d, -hi)) is written out.
//
//   pass      ONE pass over the window: a wave takes 64 consecutive columns, classifies each sample once and reads every
//             needed row element once, coalesced.  Bin, threshold, row, zone and header counts: ballots and LDS integer
//             atomics, one global integer atomic per touched word when the workgroup ends.  Grid cells: the 256 x 256 grid
//             does not fit LDS, but landing points cluster: a 32-bit LDS tile covers the 64 x 64 cells around the first
//             impact the workgroup sees (a cache, not a rule: integer adds commute, so where the tile lies cannot reach
//             the state); a cell outside it goes to L2 with a 64-bit integer atomic.  The long accumulators live in LDS:
//             every lane adds the three int64 parts of its value with LDS integer atomics (measured against a fold over the
//             wave first, which was slower); the words go to the state as they are and
//   finish    workgroup 0 propagates the carries of every accumulator (a thread each); workgroup 1 + 2 j + side settles the
//             extremes of row j: the held entries and the candidates of the pass - the lanes that beat the k-th held value
//             appended (bits, id) to a bounded list - are sorted by (key, id) in LDS and the first k kept.  A list that
//             overflowed (the first window into an empty tally) is not read: the workgroup scans the row instead, the k-th
//             value of its buffer as the admission threshold.  Sorting a set leaves no trace of the arrival order.
//   merge     dst += src word by word outside the extremes, then `finish` with src's held entries as the candidates.
// Integer adds commute and the carries are propagated once, so the state is the one the host rule gives, byte for byte.  No
// floating-point atomic anywhere; every loop is bounded.
#include <stdlib.h>

#include "erpl_host.h"

#include "erpl_tally.h"

// The two variants that were measured and rejected stay buildable for tools/bench_tally.py (experiment builds only; DESIGN.md
// section 8.14 has the numbers): ERPL_TALLY_ACC_FOLD = 1 folds the three parts of a value over the wave with a __shfl_down
// tree before lane 0 takes the LDS atomics, instead of every lane sending its own three parts (192 LDS atomics per wave,
// row and accumulator - which measured 12 - 17 % faster); ERPL_TALLY_GRID_DIRECT = 1 sends every grid cell to L2 (64-bit
// global integer atomics, no LDS tile).
#ifndef ERPL_TALLY_ACC_FOLD
#define ERPL_TALLY_ACC_FOLD 0
#endif
#ifndef ERPL_TALLY_GRID_DIRECT
#define ERPL_TALLY_GRID_DIRECT 0
#endif

namespace {

typedef unsigned long long u64;
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 512;       // of the pass: each one flushes its LDS words once
constexpr int kCand = 2048;           // entries of a candidate list
constexpr int kBuf = 1024;            // entries of the sort buffer of `finish`: a power of two, >= ERPL_TALLY_MAX_K + kBlock
constexpr int kSlots = 2 * ERPL_TALLY_MAX_ROWS;
constexpr int kTileSide = 64;         // the LDS tile of the grid: kTileSide x kTileSide cells, what fits beside the rest
constexpr int kAcc2 = 2 * ERPL_TALLY_ACC_WORDS;
constexpr int kCounters = ERPL_TALLY_HEADER_WORDS + ERPL_TALLY_MAX_ROWS * ERPL_TALLY_ROW_WORDS + ERPL_TALLY_GRID_WORDS;
constexpr int kRowCnt = ERPL_TALLY_HEADER_WORDS, kGridCnt = kRowCnt + ERPL_TALLY_MAX_ROWS * ERPL_TALLY_ROW_WORDS;
static_assert(kBuf >= ERPL_TALLY_MAX_K + kBlock && (kBuf & (kBuf - 1)) == 0, "the sort buffer");

// the workspace of the context: the spec, the fill of every candidate list, the lists ((bits, id) pairs)
struct TallyWork {
  erpl_tally_spec spec;
  unsigned int cand_count[kSlots];
  int64_t cand[kSlots][kCand][2];
};

struct TallyArgs {
  TallyWork* work;
  ErplTallyLayout L;
  int64_t* state;
  const int64_t* src;         // merge: the other state
  const double* summary;
  const int32_t* status;
  int64_t ld, n, first_id;
};

__device__ __forceinline__ void state_add(int64_t* w, int64_t v) { atomicAdd((u64*)w, (u64)v); }

// The exact value v of every lane with use into the LDS accumulator acc: its three parts as integer atomics on three
// neighbouring words.  Values of one row share an exponent, so a wave hits the same three words; the LDS unit resolves those
// adds faster than the wave fold below (the rejected variant: groups of lanes with the same first digit summed over the wave,
// lane 0 adds; at most 64 trips, every trip retires its leader).  Integer adds commute: both give the same words.
__device__ __forceinline__ void acc_fold(int64_t* acc, bool use, double v, int lane) {
  const ErplAccParts p = erpl_acc_split(use ? v : 0.0);
#if !ERPL_TALLY_ACC_FOLD
  if (use)
    for (int t = 0; t < 3; ++t)
      if (p.c[t]) atomicAdd((u64*)&acc[p.j + t], (u64)p.c[t]);
  return;
#endif
  u64 todo = __ballot(use);
  for (int trip = 0; trip < 64 && todo; ++trip) {
    const int lead = __ffsll((long long)todo) - 1;
    const int j0 = __shfl(p.j, lead);
    const bool mine = use && p.j == j0;
    long long c0 = mine ? p.c[0] : 0, c1 = mine ? p.c[1] : 0, c2 = mine ? p.c[2] : 0;
    for (int off = 32; off > 0; off >>= 1) {
      c0 += __shfl_down(c0, off);
      c1 += __shfl_down(c1, off);
      c2 += __shfl_down(c2, off);
    }
    if (lane == 0) {
      if (c0) atomicAdd((u64*)&acc[j0], (u64)c0);
      if (c1) atomicAdd((u64*)&acc[j0 + 1], (u64)c1);
      if (c2) atomicAdd((u64*)&acc[j0 + 2], (u64)c2);
    }
    todo &= ~__ballot(mine);
  }
}

// a count of the wave (uniform) into an LDS counter
__device__ __forceinline__ void count_to(u64* cnt, bool hit, int lane) {
  const u64 m = __ballot(hit);
  if (m && lane == 0) atomicAdd(cnt, (u64)__popcll(m));
}

// one bin or cell per lane with hit; a whole wave in one word is one add
template <class T>
__device__ __forceinline__ void bin_to(T* base, bool hit, int k, int lane) {
  const u64 m = __ballot(hit);
  if (m == 0ull) return;
  const int lead = __ffsll((long long)m) - 1;
  const int k0 = __shfl(k, lead);
  if (__ballot(hit && k != k0) == 0ull) {
    if (lane == lead) atomicAdd(&base[k0], (T)__popcll(m));
  } else if (hit) {
    atomicAdd(&base[k], (T)1);
  }
}

__global__ __launch_bounds__(kBlock) void erpl_tally_pass(const TallyArgs a) {
  __shared__ unsigned int s_hist[ERPL_TALLY_MAX_ROWS * ERPL_TALLY_MAX_BINS];
  __shared__ int64_t s_acc[ERPL_TALLY_MAX_ROWS * kAcc2];
  __shared__ u64 s_cnt[kCounters];
  __shared__ ErplEdges s_edges[ERPL_TALLY_MAX_ROWS + 2];
  __shared__ ErplExtreme s_thr[kSlots];
  __shared__ int s_open[kSlots], s_hoff[ERPL_TALLY_MAX_ROWS + 1];
  __shared__ double s_vx[ERPL_TALLY_MAX_VERTICES], s_vy[ERPL_TALLY_MAX_VERTICES];
  __shared__ unsigned int s_cells[kTileSide * kTileSide];
  __shared__ int s_origin;    // first cell of the tile, x * 65536 + y; -1 until the workgroup has seen an impact on the grid
  const erpl_tally_spec& s = a.work->spec;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_rows = s.n_rows, k = s.k, n_zones = s.n_zones;
  const int bins_x = s.bins_x, bins_y = s.bins_y;
  const int tile_x = bins_x < kTileSide ? bins_x : kTileSide, tile_y = bins_y < kTileSide ? bins_y : kTileSide;
  for (int t = threadIdx.x; t < kTileSide * kTileSide; t += kBlock) s_cells[t] = 0u;
  if (threadIdx.x == 0) s_origin = -1;
  const int64_t n = a.n, ld = a.ld, stride = (int64_t)gridDim.x * kBlock;

  for (int t = threadIdx.x; t < ERPL_TALLY_MAX_ROWS * ERPL_TALLY_MAX_BINS; t += kBlock) s_hist[t] = 0u;
  for (int t = threadIdx.x; t < ERPL_TALLY_MAX_ROWS * kAcc2; t += kBlock) s_acc[t] = 0;
  for (int t = threadIdx.x; t < kCounters; t += kBlock) s_cnt[t] = 0ull;
  for (int t = threadIdx.x; t < ERPL_TALLY_MAX_VERTICES; t += kBlock) { s_vx[t] = s.zone_x[t]; s_vy[t] = s.zone_y[t]; }
  if (threadIdx.x < n_rows) s_edges[threadIdx.x] = erpl_edges_of(s.lo[threadIdx.x], s.hi[threadIdx.x], s.bins[threadIdx.x]);
  if (threadIdx.x == ERPL_TALLY_MAX_ROWS) s_edges[ERPL_TALLY_MAX_ROWS] = erpl_edges_of(s.lo_x, s.hi_x, s.bins_x);
  if (threadIdx.x == ERPL_TALLY_MAX_ROWS + 1) s_edges[ERPL_TALLY_MAX_ROWS + 1] = erpl_edges_of(s.lo_y, s.hi_y, s.bins_y);
  if (threadIdx.x == 0) {
    int at = 0;
    for (int j = 0; j <= ERPL_TALLY_MAX_ROWS; ++j) { s_hoff[j] = at; if (j < n_rows) at += s.bins[j]; }
  }
  if (threadIdx.x < kSlots) {
    // the admission threshold of a side: its k-th held entry; fewer held: everything is admitted
    const int j = threadIdx.x >> 1, side = threadIdx.x & 1;
    int open = 1;
    ErplExtreme thr = {0ull, 0};
    if (j < n_rows && k > 0) {
      const int64_t* ext = a.state + a.L.ext[j];
      if (ext[side] >= k) {
        open = 0;
        const int64_t* last = ext + 2 + 2 * k * side + 2 * (k - 1);
        thr.key = erpl_extreme_key(erpl_double_of((uint64_t)last[0]), side);
        thr.id = last[1];
      }
    }
    s_open[threadIdx.x] = open;
    s_thr[threadIdx.x] = thr;
  }
  __syncthreads();

  const ErplFilter f = {s.max_apogee, s.min_apogee, s.max_range, s.max_flight_time, s.energy_apogee};
  const double* __restrict__ sum = a.summary;
  u64 head[13];   // reason[6], termination[5], status nan, incomplete: uniform over the wave
#pragma unroll
  for (int b = 0; b < 13; ++b) head[b] = 0ull;
  u64 n_valid = 0ull;
  // the loop bound is uniform over the wave: every lane takes part in every ballot and shuffle
  for (int64_t base = (int64_t)blockIdx.x * kBlock + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    const bool in = i < n;
    double apo = 0.0, rng = 0.0, ft = 0.0;
    int st = -1;
    if (in) {
      apo = sum[ERPL_SUM_APOGEE_ALT * ld + i];
      rng = sum[ERPL_SUM_RANGE * ld + i];
      ft = sum[ERPL_SUM_FLIGHT_TIME * ld + i];
      if (a.status) st = a.status[i];
    }
    const int why = in ? erpl_why_of(f, apo, rng, ft) : 0;
    const bool valid = in && why == 0;
#pragma unroll
    for (int b = 0; b < 6; ++b) head[b] += __popcll(__ballot(in && (why & (1 << b))));
    if (a.status) {
#pragma unroll
      for (int b = 0; b < 5; ++b) head[6 + b] += __popcll(__ballot(in && (st & 0xFF) == b));
      head[11] += __popcll(__ballot(in && (st & ERPL_ST_NAN)));
      head[12] += __popcll(__ballot(in && (st & ERPL_ST_INCOMPLETE)));
    }
    const u64 vm = __ballot(valid);
    n_valid += __popcll(vm);
    if (vm == 0ull) continue;
    const int64_t id = a.first_id + i;

    for (int j = 0; j < n_rows; ++j) {
      const int r = s.rows[j];
      double x = 0.0;
      if (r == ERPL_SUM_APOGEE_ALT) x = apo;
      else if (r == ERPL_SUM_RANGE) x = rng;
      else if (r == ERPL_SUM_FLIGHT_TIME) x = ft;
      else if (valid) x = sum[(int64_t)r * ld + i];
      const bool counted = valid && erpl_is_finite(x);
      if (__ballot(counted) == 0ull) continue;
      u64* cnt = s_cnt + kRowCnt + j * ERPL_TALLY_ROW_WORDS;
      const double lo = s.lo[j], hi = s.hi[j];
      const bool lt = counted && x < lo, gt = counted && x > hi, hit = counted && !lt && !gt;
      count_to(cnt + 0, counted, lane);
      count_to(cnt + 1, lt, lane);
      count_to(cnt + 2, gt, lane);
      const int nt = s.n_thresholds[j];
      for (int t = 0; t < nt; ++t) count_to(cnt + 4 + t, counted && x > s.threshold[j][t], lane);
      const int bin = hit ? erpl_bin_of(x, lo, hi, s.bins[j], s_edges[j]) : 0;
      bin_to(s_hist + s_hoff[j], hit, bin, lane);
      ErplMoment m = {0.0, 0.0, 0.0};
      const bool mom = counted && erpl_tally_moment(x, s.centre[j], &m);
      count_to(cnt + 3, counted && !mom, lane);
      acc_fold(s_acc + j * kAcc2, mom, m.d, lane);
      acc_fold(s_acc + j * kAcc2 + ERPL_TALLY_ACC_WORDS, mom, m.hi, lane);
      acc_fold(s_acc + j * kAcc2 + ERPL_TALLY_ACC_WORDS, mom && m.lo != 0.0, m.lo, lane);
      if (k > 0) {
        for (int side = 0; side < 2; ++side) {
          const int slot = 2 * j + side;
          const ErplExtreme e = {erpl_extreme_key(x, side), id};
          const bool cand = counted && (s_open[slot] || erpl_extreme_before(e, s_thr[slot]));
          const u64 cm = __ballot(cand);
          if (cm == 0ull) continue;
          const int lead = __ffsll((long long)cm) - 1;
          unsigned int at = kCand;
          if (lane == lead) {
            // a list that has overflowed is not read: no need to count further into it
            const unsigned int seen = __hip_atomic_load(&a.work->cand_count[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen <= (unsigned int)kCand) at = atomicAdd(&a.work->cand_count[slot], (unsigned int)__popcll(cm));
          }
          at = __shfl(at, lead);
          const unsigned int mine = at + (unsigned int)__popcll(cm & ((1ull << lane) - 1ull));
          if (cand && mine < (unsigned int)kCand) {
            a.work->cand[slot][mine][0] = (int64_t)erpl_bits_of(x);
            a.work->cand[slot][mine][1] = id;
          }
        }
      }
    }

    // the impact grid and the zones
    double px = 0.0, py = 0.0;
    {
      const int rx = s.row_x, ry = s.row_y;
      if (rx == ERPL_SUM_APOGEE_ALT) px = apo; else if (rx == ERPL_SUM_RANGE) px = rng; else if (rx == ERPL_SUM_FLIGHT_TIME) px = ft;
      else if (valid) px = sum[(int64_t)rx * ld + i];
      if (ry == ERPL_SUM_APOGEE_ALT) py = apo; else if (ry == ERPL_SUM_RANGE) py = rng; else if (ry == ERPL_SUM_FLIGHT_TIME) py = ft;
      else if (valid) py = sum[(int64_t)ry * ld + i];
    }
    const bool use = valid && erpl_is_finite(px) && erpl_is_finite(py);
    if (__ballot(use) == 0ull) continue;
    const bool inside = use && px >= s.lo_x && px <= s.hi_x && py >= s.lo_y && py <= s.hi_y;
    count_to(s_cnt + kGridCnt + 0, use, lane);
    count_to(s_cnt + kGridCnt + 1, use && !inside, lane);
    const int cx = inside ? erpl_bin_of(px, s.lo_x, s.hi_x, bins_x, s_edges[ERPL_TALLY_MAX_ROWS]) : 0;
    const int cy = inside ? erpl_bin_of(py, s.lo_y, s.hi_y, bins_y, s_edges[ERPL_TALLY_MAX_ROWS + 1]) : 0;
    const u64 im = __ballot(inside);
    if (im != 0ull) {
#if ERPL_TALLY_GRID_DIRECT
      bin_to((u64*)(a.state + a.L.cells), inside, cx * bins_y + cy, lane);
#else
      // the tile: centred on the first impact the workgroup sees, kept inside the grid
      const int lead = __ffsll((long long)im) - 1;
      int org = 0;
      if (lane == lead) {
        org = __hip_atomic_load(&s_origin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (org < 0) {
          int ox = cx - tile_x / 2, oy = cy - tile_y / 2;
          ox = ox < 0 ? 0 : (ox > bins_x - tile_x ? bins_x - tile_x : ox);
          oy = oy < 0 ? 0 : (oy > bins_y - tile_y ? bins_y - tile_y : oy);
          const int mine = ox * 65536 + oy;
          const int old = atomicCAS(&s_origin, -1, mine);
          org = old < 0 ? mine : old;
        }
      }
      org = __shfl(org, lead);
      const int tx = cx - (org >> 16), ty = cy - (org & 0xffff);
      const bool near = inside && tx >= 0 && tx < tile_x && ty >= 0 && ty < tile_y;
      bin_to(s_cells, near, tx * tile_y + ty, lane);
      bin_to((u64*)(a.state + a.L.cells), inside && !near, cx * bins_y + cy, lane);
#endif
    }
    for (int z = 0; z < n_zones; ++z) {
      const int v0 = s.zone_first[z], v1 = s.zone_first[z + 1];   // the host has checked 0 <= v0, v0 + 3 <= v1 <= 256
      bool c = false;
      for (int vi = v0, vj = v1 - 1; vi < v1; vj = vi++)
        if (erpl_zone_flips(px, py, s_vx[vi], s_vy[vi], s_vx[vj], s_vy[vj])) c = !c;
      count_to(s_cnt + kGridCnt + 2 + z, use && c, lane);
    }
  }
  if (lane == 0) {
    if (n_valid) atomicAdd(&s_cnt[1], n_valid);
#pragma unroll
    for (int b = 0; b < 13; ++b)
      if (head[b]) atomicAdd(&s_cnt[2 + b], head[b]);
  }
  __syncthreads();

  // one global integer atomic per touched word
  if (blockIdx.x == 0 && threadIdx.x == 0) state_add(a.state, n);
  for (int t = threadIdx.x; t < ERPL_TALLY_HEADER_WORDS; t += kBlock)
    if (s_cnt[t]) state_add(a.state + t, (int64_t)s_cnt[t]);
  for (int t = threadIdx.x; t < n_rows * ERPL_TALLY_ROW_WORDS; t += kBlock)
    if (s_cnt[kRowCnt + t]) state_add(a.state + a.L.row[t / ERPL_TALLY_ROW_WORDS] + t % ERPL_TALLY_ROW_WORDS, (int64_t)s_cnt[kRowCnt + t]);
  for (int t = threadIdx.x; t < ERPL_TALLY_GRID_WORDS; t += kBlock)
    if (s_cnt[kGridCnt + t]) state_add(a.state + a.L.grid + t, (int64_t)s_cnt[kGridCnt + t]);
  if (s_origin >= 0)
    for (int t = threadIdx.x; t < tile_x * tile_y; t += kBlock)
      if (s_cells[t]) state_add(a.state + a.L.cells + (int64_t)((s_origin >> 16) + t / tile_y) * bins_y + (s_origin & 0xffff) + t % tile_y, (int64_t)s_cells[t]);
  for (int j = 0; j < n_rows; ++j) {
    const int bins = s.bins[j];
    for (int t = threadIdx.x; t < bins; t += kBlock) {
      const unsigned int c = s_hist[s_hoff[j] + t];
      if (c) state_add(a.state + a.L.hist[j] + t, (int64_t)c);
    }
    for (int t = threadIdx.x; t < kAcc2; t += kBlock) {
      const int64_t v = s_acc[j * kAcc2 + t];
      if (v) state_add(a.state + a.L.acc[j] + t, v);
    }
  }
}

// ---- finish.  MERGE = false: behind erpl_tally_pass; true: behind erpl_tally_merge_words.
__device__ __forceinline__ void sort_buffer(u64* key, int64_t* id) {
  for (int span = 2; span <= kBuf; span <<= 1)
    for (int step = span >> 1; step > 0; step >>= 1) {
      for (int t = threadIdx.x; t < kBuf; t += kBlock) {
        const int u = t ^ step;
        if (u > t) {
          const ErplExtreme x = {key[t], id[t]}, y = {key[u], id[u]};
          const bool up = (t & span) == 0;
          if (up ? erpl_extreme_before(y, x) : erpl_extreme_before(x, y)) {
            key[t] = y.key; id[t] = y.id;
            key[u] = x.key; id[u] = x.id;
          }
        }
      }
      __syncthreads();
    }
}

template <bool MERGE>
__global__ __launch_bounds__(kBlock) void erpl_tally_finish(const TallyArgs a) {
  __shared__ u64 s_key[kBuf];
  __shared__ int64_t s_id[kBuf];
  __shared__ int s_fill, s_full;
  __shared__ ErplExtreme s_thr;
  const erpl_tally_spec& s = a.work->spec;
  const int n_rows = s.n_rows, k = s.k;
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < 2 * n_rows)
      erpl_acc_normalise(a.state + a.L.acc[threadIdx.x >> 1] + (threadIdx.x & 1) * ERPL_TALLY_ACC_WORDS);
    return;
  }
  const int slot = blockIdx.x - 1, j = slot >> 1, side = slot & 1;   // the host launches 1 + 2 n_rows workgroups, k > 0
  int64_t* ext = a.state + a.L.ext[j];
  int64_t* list = ext + 2 + 2 * k * side;
  const u64 none_key = ~0ull;   // behind every finite value's key on either side
  const int64_t none_id = INT64_MAX;

  // sorts the buffer, keeps the first k and makes the k-th the threshold; every thread calls it
  auto settle = [&]() {
    __syncthreads();
    const int fill = s_fill;
    for (int t = threadIdx.x; t < kBuf; t += kBlock)
      if (t >= fill) { s_key[t] = none_key; s_id[t] = none_id; }
    __syncthreads();
    sort_buffer(s_key, s_id);
    if (threadIdx.x == 0) {
      s_fill = fill < k ? fill : k;
      s_full = fill >= k;
      if (fill >= k) { s_thr.key = s_key[k - 1]; s_thr.id = s_id[k - 1]; }
    }
    __syncthreads();
  };
  // one candidate per thread (has = false: none): into the buffer if it beats the threshold.  Every thread calls it.
  auto offer = [&](bool has, uint64_t bits, int64_t id) {
    const bool crowded = s_fill + kBlock > kBuf;
    __syncthreads();   // nobody appends before everybody has read the fill
    if (crowded) settle();
    if (has) {
      const ErplExtreme e = {erpl_extreme_key(erpl_double_of(bits), side), id};
      if (!s_full || erpl_extreme_before(e, s_thr)) {
        const int at = atomicAdd(&s_fill, 1);
        s_key[at] = e.key; s_id[at] = e.id;
      }
    }
    __syncthreads();
  };

  int64_t held = ext[side];
  held = held < 0 ? 0 : (held > k ? k : held);
  for (int t = threadIdx.x; t < (int)held; t += kBlock) {
    s_key[t] = erpl_extreme_key(erpl_double_of((uint64_t)list[2 * t]), side);
    s_id[t] = list[2 * t + 1];
  }
  if (threadIdx.x == 0) {
    s_fill = (int)held;
    s_full = held >= k;
    if (held >= k) { s_thr.key = erpl_extreme_key(erpl_double_of((uint64_t)list[2 * (k - 1)]), side); s_thr.id = list[2 * (k - 1) + 1]; }
  }
  __syncthreads();

  const int64_t* from;
  int64_t m;
  bool scan = false;
  if (MERGE) {
    from = a.src + a.L.ext[j] + 2 + 2 * k * side;
    m = a.src[a.L.ext[j] + side];
    m = m < 0 ? 0 : (m > k ? k : m);
  } else {
    from = &a.work->cand[slot][0][0];
    m = a.work->cand_count[slot];
    if (m > kCand) { scan = true; m = a.n; }
  }
  if (!scan) {
    for (int64_t base = 0; base < m; base += kBlock) {
      const int64_t e = base + threadIdx.x;
      const bool has = e < m;
      offer(has, has ? (uint64_t)from[2 * e] : 0ull, has ? from[2 * e + 1] : 0);
    }
  } else {
    // the list overflowed: the row itself, with the rule of the pass
    const ErplFilter f = {s.max_apogee, s.min_apogee, s.max_range, s.max_flight_time, s.energy_apogee};
    const int r = s.rows[j];
    for (int64_t base = 0; base < m; base += kBlock) {
      const int64_t i = base + threadIdx.x;
      bool has = false;
      double x = 0.0;
      if (i < m) {
        const int why = erpl_why_of(f, a.summary[ERPL_SUM_APOGEE_ALT * a.ld + i], a.summary[ERPL_SUM_RANGE * a.ld + i],
                                    a.summary[ERPL_SUM_FLIGHT_TIME * a.ld + i]);
        x = a.summary[(int64_t)r * a.ld + i];
        has = why == 0 && erpl_is_finite(x);
      }
      offer(has, erpl_bits_of(x), a.first_id + i);
    }
  }
  settle();
  const int fill = s_fill;
  for (int t = threadIdx.x; t < k; t += kBlock) {
    list[2 * t] = t < fill ? (int64_t)erpl_extreme_bits(s_key[t], side) : 0;
    list[2 * t + 1] = t < fill ? s_id[t] : 0;
  }
  if (threadIdx.x == 0) {
    ext[side] = fill;
    if (!MERGE) a.work->cand_count[slot] = 0u;   // for the next pass on this context
  }
}

__global__ __launch_bounds__(kBlock) void erpl_tally_merge_words(const TallyArgs a) {
  const erpl_tally_spec& s = a.work->spec;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < a.L.words; w += stride)
    if (!erpl_tally_is_extreme(a.L, s.n_rows, s.k, w)) a.state[w] += a.src[w];
}

// ---- host

#define NEED(p, name) do { if (!(p)) return erpl_fail(ERPL_ERR_INVALID, name " is NULL"); } while (0)

// the refusals of a spec, in the order of the header (erpl_tally_check_spec), as texts
int spec_check(const erpl_tally_spec* s) {
  NEED(s, "spec");
  int at = -1;
  const int rc = erpl_tally_check_spec(*s, &at);
  static const char* bound[5] = {"max_apogee", "min_apogee", "max_range", "max_flight_time", "energy_apogee"};
  switch (rc) {
    case 0: return ERPL_OK;
    case ERPL_TALLY_BAD_BOUND: return erpl_fail(ERPL_ERR_INVALID, "spec->%s is NaN", bound[at]);
    case ERPL_TALLY_BAD_N_ROWS: return erpl_fail(ERPL_ERR_INVALID, "spec->n_rows = %d outside 0..%d", s->n_rows, ERPL_TALLY_MAX_ROWS);
    case ERPL_TALLY_BAD_ROW: return erpl_fail(ERPL_ERR_INVALID, "spec->rows[%d] = %d outside 0..%d", at, s->rows[at], ERPL_SUMMARY_DIM - 1);
    case ERPL_TALLY_ROW_TWICE: return erpl_fail(ERPL_ERR_INVALID, "spec->rows[%d] = %d is listed twice", at, s->rows[at]);
    case ERPL_TALLY_BAD_BINS: return erpl_fail(ERPL_ERR_INVALID, "spec->bins[%d] = %d outside 1..%d", at, s->bins[at], ERPL_TALLY_MAX_BINS);
    case ERPL_TALLY_BAD_RANGE:
      return erpl_fail(ERPL_ERR_INVALID, "spec->lo[%d] = %g, spec->hi[%d] = %g: not a finite range with lo < hi", at, s->lo[at], at, s->hi[at]);
    case ERPL_TALLY_BAD_CENTRE: return erpl_fail(ERPL_ERR_INVALID, "spec->centre[%d] = %g is not finite", at, s->centre[at]);
    case ERPL_TALLY_BAD_N_THRESHOLDS:
      return erpl_fail(ERPL_ERR_INVALID, "spec->n_thresholds[%d] = %d outside 0..%d", at, s->n_thresholds[at], ERPL_TALLY_MAX_THRESHOLDS);
    case ERPL_TALLY_BAD_THRESHOLD: return erpl_fail(ERPL_ERR_INVALID, "spec->threshold[%d] holds a NaN", at);
    case ERPL_TALLY_BAD_K: return erpl_fail(ERPL_ERR_INVALID, "spec->k = %d outside 0..%d", s->k, ERPL_TALLY_MAX_K);
    case ERPL_TALLY_BAD_N_Q: return erpl_fail(ERPL_ERR_INVALID, "spec->n_q = %d outside 0..%d", s->n_q, ERPL_TALLY_MAX_Q);
    case ERPL_TALLY_BAD_Q: return erpl_fail(ERPL_ERR_INVALID, "spec->q[%d] = %g outside [0, 1]", at, s->q[at]);
    case ERPL_TALLY_BAD_ROW_X: return erpl_fail(ERPL_ERR_INVALID, "spec->row_x = %d outside 0..%d", s->row_x, ERPL_SUMMARY_DIM - 1);
    case ERPL_TALLY_BAD_ROW_Y: return erpl_fail(ERPL_ERR_INVALID, "spec->row_y = %d outside 0..%d", s->row_y, ERPL_SUMMARY_DIM - 1);
    case ERPL_TALLY_ROW_XY_SAME: return erpl_fail(ERPL_ERR_INVALID, "spec->row_y = %d is listed twice (row_x)", s->row_y);
    case ERPL_TALLY_BAD_BINS_X: return erpl_fail(ERPL_ERR_INVALID, "spec->bins_x = %d outside 1..%d", s->bins_x, ERPL_TALLY_MAX_GRID);
    case ERPL_TALLY_BAD_BINS_Y: return erpl_fail(ERPL_ERR_INVALID, "spec->bins_y = %d outside 1..%d", s->bins_y, ERPL_TALLY_MAX_GRID);
    case ERPL_TALLY_BAD_RANGE_X:
      return erpl_fail(ERPL_ERR_INVALID, "spec->lo_x = %g, spec->hi_x = %g: not a finite range with lo < hi", s->lo_x, s->hi_x);
    case ERPL_TALLY_BAD_RANGE_Y:
      return erpl_fail(ERPL_ERR_INVALID, "spec->lo_y = %g, spec->hi_y = %g: not a finite range with lo < hi", s->lo_y, s->hi_y);
    case ERPL_TALLY_BAD_N_ZONES: return erpl_fail(ERPL_ERR_INVALID, "spec->n_zones = %d outside 0..%d", s->n_zones, ERPL_TALLY_MAX_ZONES);
    case ERPL_TALLY_BAD_ZONE_FIRST:
      return erpl_fail(ERPL_ERR_INVALID, "spec->zone_first: zone %d does not start at vertex 0 or ends before it starts", at);
    case ERPL_TALLY_ZONE_SHORT: return erpl_fail(ERPL_ERR_INVALID, "spec->zone_first: zone %d has fewer than 3 vertices, a polygon needs 3", at);
    case ERPL_TALLY_ZONE_LONG: return erpl_fail(ERPL_ERR_INVALID, "spec->zone_first: more than %d vertices together (zone %d)", ERPL_TALLY_MAX_VERTICES, at);
    default: return erpl_fail(ERPL_ERR_INVALID, "spec->zone_x[%d] = %g, spec->zone_y[%d] = %g: not a finite vertex", at, s->zone_x[at], at, s->zone_y[at]);
  }
}

int window_check(const int64_t* state, const double* summary, int64_t ld, int64_t n, int64_t first_id) {
  NEED(state, "state");
  NEED(summary, "summary");
  if (n <= 0) return erpl_fail(ERPL_ERR_INVALID, "n = %lld: need at least one sample", (long long)n);
  // a word of an accumulator takes 2^31 parts, a 32-bit LDS bin 2^32 counts, before the carries of a window are propagated
  if (n > INT32_MAX) return erpl_fail(ERPL_ERR_INVALID, "n = %lld exceeds 2^31 - 1 columns per call", (long long)n);
  if (ld < n) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below n = %lld", (long long)ld, (long long)n);
  if (first_id < 0) return erpl_fail(ERPL_ERR_INVALID, "first_id = %lld is negative", (long long)first_id);
  if (first_id > INT64_MAX - n) return erpl_fail(ERPL_ERR_INVALID, "first_id + n = %lld + %lld overflows", (long long)first_id, (long long)n);
  return ERPL_OK;
}

int result_finish(int rc, const erpl_tally* result) {
  if (rc != 0) return erpl_fail(ERPL_ERR_INVALID, "state: a count word is negative or has passed 2^62");
  if (result->n_incomplete > 0)
    return erpl_fail(ERPL_ERR_INCOMPLETE, "%lld sample(s) carry ERPL_ST_INCOMPLETE: they were never integrated", (long long)result->n_incomplete);
  return ERPL_OK;
}

// The workspace and the spec on the device.  A spec other than the one there waits for the device first - an earlier call,
// on whatever stream, may still read the old one - and for its own upload, so that a later call on another stream finds it.
int tally_ready(erpl_ctx* c, const erpl_tally_spec* spec, hipStream_t st, TallyArgs* a) {
  HIP_TRY(hipSetDevice(c->device));
  const bool first = c->tally.buf == nullptr;
  ERPL_TRY(c->tally.first_use());
  ERPL_TRY(c->tally.grow(sizeof(TallyWork)));
  TallyWork* w = (TallyWork*)c->tally.buf;
  if (first || memcmp(c->tally.host, spec, sizeof(*spec)) != 0) {
    HIP_TRY(hipDeviceSynchronize());
    if (first) HIP_TRY(hipMemsetAsync(w->cand_count, 0, sizeof(w->cand_count), st));
    memcpy(c->tally.host, spec, sizeof(*spec));
    HIP_TRY(hipMemcpyAsync(&w->spec, c->tally.host, sizeof(*spec), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  *a = TallyArgs{};
  a->work = w;
  a->L = erpl_tally_layout(*spec);
  return ERPL_OK;
}

}  // namespace

extern "C" {

int erpl_mc_tally_defaults(erpl_tally_spec* spec) {
  NEED(spec, "spec");
  memset(spec, 0, sizeof(*spec));
  erpl_analysis_spec ana;
  ERPL_TRY(erpl_mc_analysis_defaults(&ana));
  spec->max_apogee = ana.max_apogee; spec->min_apogee = ana.min_apogee; spec->max_range = ana.max_range;
  spec->max_flight_time = ana.max_flight_time; spec->energy_apogee = ana.energy_apogee;
  spec->n_rows = 3;
  const int32_t rows[3] = {ERPL_SUM_APOGEE_ALT, ERPL_SUM_RANGE, ERPL_SUM_FLIGHT_TIME};
  const double hi[3] = {ana.max_apogee, ana.max_range, ana.max_flight_time};
  for (int j = 0; j < 3; ++j) {
    spec->rows[j] = rows[j];
    spec->bins[j] = 1000;
    spec->lo[j] = 0.0; spec->hi[j] = hi[j];
    spec->centre[j] = 0.5 * hi[j];
  }
  spec->k = 16;
  spec->n_q = ana.n_q;
  for (int q = 0; q < ana.n_q; ++q) spec->q[q] = ana.q[q];
  spec->row_x = ERPL_SUM_IMPACT_X; spec->row_y = ERPL_SUM_IMPACT_Y;
  spec->bins_x = spec->bins_y = 128;
  spec->lo_x = spec->lo_y = -200000.0;
  spec->hi_x = spec->hi_y = 200000.0;
  return ERPL_OK;
}

int erpl_mc_tally_words(const erpl_tally_spec* spec, int64_t* words) {
  ERPL_TRY(spec_check(spec));
  NEED(words, "words");
  *words = erpl_tally_layout(*spec).words;
  return ERPL_OK;
}

int erpl_mc_tally_add_host(const erpl_tally_spec* spec, int64_t* state, const double* summary, int64_t ld, const int32_t* status,
                           int64_t n, int64_t first_id) {
  ERPL_TRY(spec_check(spec));
  ERPL_TRY(window_check(state, summary, ld, n, first_id));
  erpl_tally_add_rule(*spec, state, summary, ld, status, n, first_id);
  return ERPL_OK;
}

int erpl_mc_tally_merge_host(const erpl_tally_spec* spec, int64_t* dst, const int64_t* src) {
  ERPL_TRY(spec_check(spec));
  NEED(dst, "dst");
  NEED(src, "src");
  erpl_tally_merge_rule(*spec, dst, src);
  return ERPL_OK;
}

int erpl_mc_tally_result_host(const erpl_tally_spec* spec, const int64_t* state, erpl_tally* result, int64_t* hist_counts,
                              int64_t* grid_counts) {
  ERPL_TRY(spec_check(spec));
  NEED(state, "state");
  NEED(result, "result");
  return result_finish(erpl_tally_result_rule(*spec, state, result, hist_counts, grid_counts), result);
}

int erpl_mc_tally_add(erpl_ctx* c, const erpl_tally_spec* spec, int64_t* state, const double* summary, int64_t ld,
                      const int32_t* status, int64_t n, int64_t first_id, void* stream) {
  ERPL_TRY(spec_check(spec));
  ERPL_TRY(window_check(state, summary, ld, n, first_id));
  NEED(c, "ctx");
  const hipStream_t st = (hipStream_t)stream;
  TallyArgs a;
  ERPL_TRY(tally_ready(c, spec, st, &a));
  a.state = state; a.summary = summary; a.status = status; a.ld = ld; a.n = n; a.first_id = first_id;
  const int64_t want = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(erpl_tally_pass, dim3((unsigned)(want < kMaxBlocks ? want : kMaxBlocks)), dim3(kBlock), 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(erpl_tally_finish<false>, dim3(spec->k > 0 ? 1u + 2u * (unsigned)spec->n_rows : 1u), dim3(kBlock), 0, st, a);
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

int erpl_mc_tally_merge(erpl_ctx* c, const erpl_tally_spec* spec, int64_t* dst, const int64_t* src, void* stream) {
  ERPL_TRY(spec_check(spec));
  NEED(dst, "dst");
  NEED(src, "src");
  NEED(c, "ctx");
  const hipStream_t st = (hipStream_t)stream;
  TallyArgs a;
  ERPL_TRY(tally_ready(c, spec, st, &a));
  a.state = dst; a.src = src;
  const int64_t want = (a.L.words + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(erpl_tally_merge_words, dim3((unsigned)(want < kMaxBlocks ? want : kMaxBlocks)), dim3(kBlock), 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(erpl_tally_finish<true>, dim3(spec->k > 0 ? 1u + 2u * (unsigned)spec->n_rows : 1u), dim3(kBlock), 0, st, a);
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

int erpl_mc_tally_result(erpl_ctx* c, const erpl_tally_spec* spec, const int64_t* state, erpl_tally* result, int64_t* hist_counts,
                         int64_t* grid_counts, void* stream) {
  ERPL_TRY(spec_check(spec));
  NEED(state, "state");
  NEED(result, "result");
  NEED(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  // (malloc, not a container: no exception may cross the C boundary)
  const size_t bytes = (size_t)erpl_tally_layout(*spec).words * sizeof(int64_t);
  int64_t* host = (int64_t*)malloc(bytes);
  if (!host) return erpl_fail(ERPL_ERR_INTERNAL, "out of host memory for the %zu bytes of the state", bytes);
  hipError_t e = hipMemcpyAsync(host, state, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) {
    free(host);
    return erpl_fail(ERPL_ERR_HIP, "copy of the state: %s", hipGetErrorString(e));
  }
  const int rc = erpl_tally_result_rule(*spec, host, result, hist_counts, grid_counts);
  free(host);
  return result_finish(rc, result);
}

}  // extern "C"
