// erpl_stat_layout.h — how erpl_mc_correlation, erpl_mc_bootstrap, erpl_mc_impact_density, erpl_mc_sobol,
// erpl_mc_dependence, erpl_mc_compare, erpl_mc_surrogate, erpl_mc_reweight, erpl_mc_impact_density_weighted and erpl_mc_corridor_drivers cut the device buffer each of them grows into pieces: pure functions
// of the call's sizes (no HIP; the scratch size of the rocPRIM calls comes in as a number), so that tests/test_stat_layout.py,
// tests/test_dependence_layout.py, tests/test_compare_layout.py and tests/test_surrogate_abi.py check every offset on the CPU, through
// erpl_stat_layout_table, before a kernel writes through one.  Every piece starts at a multiple of 256 bytes; `need` is the
// end of the last one.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "erpl_tables.h"

inline size_t erpl_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The pieces of a buffer, one after the other: take(bytes) is where the next one starts (no bytes: what the caller keeps).
struct ErplCarve {
  size_t at = 0, end = 0;   // where the next piece starts, where the last one ends
  size_t take(size_t bytes) {
    end = at + bytes;
    at = erpl_align256(end);
    return end - bytes;
  }
};
// the scratch a rocPRIM call asked for as the piece it gets, and is told it has: never empty, whole lines of 256 bytes
inline size_t erpl_scratch_piece(size_t temp_bytes) { return erpl_align256(temp_bytes < 256 ? 256 : temp_bytes); }

// erpl_mc_correlation: [keys 2n u64][ranks V n doubles unless the caller keeps them][idx 2n u32][scratch of the sort] - these
// four with spec->ranks only - [pop n bytes]
struct ErplCorrLayout { size_t keys, ranks, idx, temp, pop, temp_bytes, need; };
inline ErplCorrLayout erpl_corr_layout(int64_t n, int V, bool ranks, bool caller_keeps_ranks, size_t temp_bytes) {
  const size_t un = (size_t)n;
  ErplCarve c;
  ErplCorrLayout l = {};
  if (ranks) {
    l.keys = c.take(16 * un);
    l.ranks = c.take(caller_keeps_ranks ? 0 : 8 * un * (size_t)V);
    l.idx = c.take(8 * un);
    l.temp_bytes = erpl_scratch_piece(temp_bytes);
    l.temp = c.take(l.temp_bytes);
  }
  l.pop = c.take(un);
  l.need = c.end;
  return l;
}

// erpl_mc_bootstrap: [pop n bytes][src n u32][count][x R rows of n doubles][sorted the same][pos R rows of n u32][keys 2n u64]
// [idx 2n u32][scratch of the select / the sort][zero bytes B][replicates n_stats B doubles unless the caller keeps them]
struct ErplBootLayout {
  size_t pop, src, count, x[ERPL_BOOT_MAX_ROWS], sorted[ERPL_BOOT_MAX_ROWS], pos[ERPL_BOOT_MAX_ROWS], keys, idx, temp, zero, rep,
      temp_bytes, need;
};
inline ErplBootLayout erpl_boot_layout(int64_t n, int R, int n_stats, int B, bool caller_keeps_replicates, size_t temp_bytes) {
  const size_t un = (size_t)n, uB = (size_t)B;
  ErplCarve c;
  ErplBootLayout l = {};
  l.pop = c.take(un);
  l.src = c.take(4 * un);
  l.count = c.take(8);
  for (int j = 0; j < R; ++j) l.x[j] = c.take(8 * un);
  for (int j = 0; j < R; ++j) l.sorted[j] = c.take(8 * un);
  for (int j = 0; j < R; ++j) l.pos[j] = c.take(4 * un);
  l.keys = c.take(16 * un);
  l.idx = c.take(8 * un);
  l.temp_bytes = erpl_scratch_piece(temp_bytes);
  l.temp = c.take(l.temp_bytes);
  l.zero = c.take(uB);
  l.rep = c.take(caller_keeps_replicates ? 0 : 8 * uB * (size_t)n_stats);
  l.need = c.end;
  return l;
}

// erpl_mc_impact_density: [pop n bytes][src n u32][count][scratch of the select][points n (x, y), then (u, v)][nodes (u, v)]
// [node densities][the sample row, if there is one and the caller does not keep it][partial sums: at most
// ERPL_DENS_TARGET_BLOCKS * ERPL_DENS_TILE + queries doubles (erpl_dens_slices), queries = the nodes or the samples]
struct ErplDensLayout { size_t pop, src, count, temp, pts, nodes, dens, row, part, temp_bytes, need; };
inline ErplDensLayout erpl_dens_layout(int64_t n, int64_t nodes, bool want_samples, bool caller_keeps_row, size_t temp_bytes) {
  const size_t un = (size_t)n, un_nodes = (size_t)nodes;
  ErplCarve c;
  ErplDensLayout l = {};
  l.pop = c.take(un);
  l.src = c.take(4 * un);
  l.count = c.take(8);
  l.temp_bytes = erpl_scratch_piece(temp_bytes);
  l.temp = c.take(l.temp_bytes);
  l.pts = c.take(16 * un);
  l.nodes = c.take(16 * un_nodes);
  l.dens = c.take(8 * un_nodes);
  l.row = c.take(want_samples && !caller_keeps_row ? 8 * un : 0);
  const size_t queries = want_samples && un > un_nodes ? un : un_nodes;
  l.part = c.take(8 * ((size_t)ERPL_DENS_TARGET_BLOCKS * ERPL_DENS_TILE + queries));
  l.need = c.end;
  return l;
}

// erpl_mc_impact_density_weighted: the pieces of erpl_mc_impact_density with the scaled weights of the counted points behind
// the points: [pop n bytes][src n u32][count][scratch of the select][points n (x, y), then (u, v)][ws n doubles][nodes (u, v)]
// [node densities][the sample row, if there is one and the caller does not keep it][partial sums as in erpl_dens_layout]
struct ErplDensWLayout { size_t pop, src, count, temp, pts, ws, nodes, dens, row, part, temp_bytes, need; };
inline ErplDensWLayout erpl_densw_layout(int64_t n, int64_t nodes, bool want_samples, bool caller_keeps_row, size_t temp_bytes) {
  const size_t un = (size_t)n, un_nodes = (size_t)nodes;
  ErplCarve c;
  ErplDensWLayout l = {};
  l.pop = c.take(un);
  l.src = c.take(4 * un);
  l.count = c.take(8);
  l.temp_bytes = erpl_scratch_piece(temp_bytes);
  l.temp = c.take(l.temp_bytes);
  l.pts = c.take(16 * un);
  l.ws = c.take(8 * un);
  l.nodes = c.take(16 * un_nodes);
  l.dens = c.take(8 * un_nodes);
  l.row = c.take(want_samples && !caller_keeps_row ? 8 * un : 0);
  const size_t queries = want_samples && un > un_nodes ? un : un_nodes;
  l.part = c.take(8 * ((size_t)ERPL_DENS_TARGET_BLOCKS * ERPL_DENS_TILE + queries));
  l.need = c.end;
  return l;
}

// erpl_mc_sobol over n design rows, k factors, R output rows: [pop R rows of n bytes, row r at pop + r n][src R rows of n u32]
// [counts R u64][rec R rows of n (k + 2) doubles][scratch of the select][replicates R (2 + 2 k) B doubles unless the caller
// keeps them]
struct ErplSobolLayout {
  size_t pop, src[ERPL_SOBOL_MAX_ROWS], count, rec[ERPL_SOBOL_MAX_ROWS], temp, rep, temp_bytes, need;
};
inline ErplSobolLayout erpl_sobol_layout(int64_t n, int k, int R, int B, bool caller_keeps_replicates, size_t temp_bytes) {
  const size_t un = (size_t)n, uB = (size_t)B, uk = (size_t)k, uR = (size_t)R;
  ErplCarve c;
  ErplSobolLayout l = {};
  l.pop = c.take(uR * un);
  for (int j = 0; j < R; ++j) l.src[j] = c.take(4 * un);
  l.count = c.take(8 * uR);
  for (int j = 0; j < R; ++j) l.rec[j] = c.take(8 * un * (uk + 2));
  l.temp_bytes = erpl_scratch_piece(temp_bytes);
  l.temp = c.take(l.temp_bytes);
  l.rep = c.take(caller_keeps_replicates ? 0 : 8 * uB * uR * (2 + 2 * uk));
  l.need = c.end;
  return l;
}

// erpl_mc_dependence over n samples, F factors, R rows, M classes, H cells, P shifts: [pop n bytes][src n u32][count][yd R rows
// of n doubles][xc F rows of x_stride class bytes][yext R rows of y_stride cell bytes, extended: 2 n + 32 of them are
// written][keys 2n u64][idx 2n u32][scratch of the select / the sort][cstat R F M 6 doubles][tab R F M H int64][null
// R F 4 P doubles].  The strides are multiples of 16: the table kernel reads 16 class bytes per load.
struct ErplDepLayout {
  size_t pop, src, count, yd[ERPL_DEP_MAX_ROWS], xc, yext, keys, idx, temp, cstat, tab, null, x_stride, y_stride, temp_bytes, need;
};
inline ErplDepLayout erpl_dep_layout(int64_t n, int F, int R, int M, int H, int P, size_t temp_bytes) {
  const size_t un = (size_t)n, pairs = (size_t)F * (size_t)R;
  ErplCarve c;
  ErplDepLayout l = {};
  l.pop = c.take(un);
  l.src = c.take(4 * un);
  l.count = c.take(8);
  for (int j = 0; j < R; ++j) l.yd[j] = c.take(8 * un);
  l.x_stride = (un + 15) & ~(size_t)15;
  l.y_stride = (2 * un + 32 + 15) & ~(size_t)15;
  l.xc = c.take(l.x_stride * (size_t)F);
  l.yext = c.take(l.y_stride * (size_t)R);
  l.keys = c.take(16 * un);
  l.idx = c.take(8 * un);
  l.temp_bytes = erpl_scratch_piece(temp_bytes);
  l.temp = c.take(l.temp_bytes);
  l.cstat = c.take(8 * 6 * pairs * (size_t)M);
  l.tab = c.take(8 * pairs * (size_t)M * (size_t)H);
  l.null = c.take(8 * 4 * pairs * (size_t)P);
  l.need = c.end;
  return l;
}

// erpl_mc_surrogate over n samples, V variables, R rows, P terms (cols = P + R): [pop n bytes][src n u32][count][scratch of the
// select][model: the four tables, 32 kind bytes, P terms of 8 bytes, R P coefficients][psi cols rows of ld doubles, ld = the
// members of a chunk: min(ERPL_SUR_CHUNK, n) rounded up to ERPL_SUR_KT][part slices pairs tiles of 128 x 128 doubles, slices =
// erpl_sur_max_slices(ld, P): the most that ANY chunk of at most ld members is cut into][gram cols cols doubles][yhat R rows
// of n doubles].
// erpl_mc_surrogate_predict needs the model piece alone: erpl_sur_model_bytes.
struct ErplSurLayout {
  size_t pop, src, count, temp, model, psi, part, gram, yhat, temp_bytes, need;
  size_t m_kinds, m_terms, m_coef, model_bytes;   // within the model piece (the tables at 0)
  int64_t ld;
  int slices;
};
inline void erpl_sur_model_pieces(int R, int P, ErplSurLayout* l) {
  l->m_kinds = 4 * 8 * (ERPL_SUR_MAX_DEGREE + 1);
  l->m_terms = l->m_kinds + ERPL_SUR_MAX_VARS;
  l->m_coef = l->m_terms + 8 * (size_t)P;
  l->model_bytes = l->m_coef + 8 * (size_t)R * (size_t)P;
}
inline ErplSurLayout erpl_sur_layout(int64_t n, int R, int P, size_t temp_bytes) {
  const size_t un = (size_t)n, cols = (size_t)(P + R);
  ErplCarve c;
  ErplSurLayout l = {};
  erpl_sur_model_pieces(R, P, &l);
  l.ld = ((n < ERPL_SUR_CHUNK ? n : ERPL_SUR_CHUNK) + ERPL_SUR_KT - 1) / ERPL_SUR_KT * ERPL_SUR_KT;
  l.slices = erpl_sur_max_slices(l.ld, P);
  l.pop = c.take(un);
  l.src = c.take(4 * un);
  l.count = c.take(8);
  l.temp_bytes = erpl_scratch_piece(temp_bytes);
  l.temp = c.take(l.temp_bytes);
  l.model = c.take(l.model_bytes);
  l.psi = c.take(8 * cols * (size_t)l.ld);
  l.part = c.take(8 * (size_t)l.slices * (size_t)erpl_sur_pairs((int)cols) * ERPL_SUR_TILE * ERPL_SUR_TILE);
  l.gram = c.take(8 * cols * cols);
  l.yhat = c.take(8 * un * (size_t)R);
  l.need = c.end;
  return l;
}

// erpl_mc_compare keeps TWO buffers, because the pooled size N = m_a + m_b is known only after the populations are counted.
// The population buffer, a function of (n_a, n_b): [pop_a n_a bytes][src_a n_a u32][pop_b n_b bytes][src_b n_b u32][counts 2 u64]
// [scratch of the select]; pop_need is its end.
// The pooled buffer, a function of (N, R, P, bivariate): [val R rows of N doubles][xy N (x, y), bivariate][keys 2N u64][idx 2N u32]
// [scratch of the sort][sidx R rows of N u32][r2e R rows of N u64][thr words 64 (key, index)][bits N wb u64][cnt chunks wb 64
// u32][part chunks wb 64 records of 64 bytes][rank R words 64 records][at_value R doubles][epart tiles slices wb 64 3 doubles,
// bivariate][eout words 64 3 doubles]; words = ceil((P + 1) / 64), wb = erpl_cmp_block_words, chunks = erpl_cmp_chunks, tiles =
// ceil(N / ERPL_CMP_TILE), slices = erpl_cmp_slices (erpl_tables.h).  N == 0: the pooled buffer is empty, need = 0.
struct ErplCompareLayout {
  size_t pop_a, src_a, pop_b, src_b, count, sel_temp, sel_bytes, pop_need;
  size_t val[ERPL_CMP_MAX_ROWS], xy, keys, idx, temp, sidx[ERPL_CMP_MAX_ROWS], r2e[ERPL_CMP_MAX_ROWS], thr, bits, cnt, part, rank,
      at_value, epart, eout, temp_bytes, need;
  int words, wb, chunks, slices;
};
inline ErplCompareLayout erpl_compare_layout(int64_t n_a, int64_t n_b, int64_t N, int R, int P, bool bivariate, size_t select_bytes,
                                             size_t sort_bytes) {
  const size_t ua = (size_t)n_a, ub = (size_t)n_b, uN = (size_t)N, uR = (size_t)R;
  ErplCompareLayout l = {};
  ErplCarve c;
  l.pop_a = c.take(ua);
  l.src_a = c.take(4 * ua);
  l.pop_b = c.take(ub);
  l.src_b = c.take(4 * ub);
  l.count = c.take(16);
  l.sel_bytes = erpl_scratch_piece(select_bytes);
  l.sel_temp = c.take(l.sel_bytes);
  l.pop_need = c.end;
  l.words = erpl_cmp_words(P);
  if (N <= 0) return l;
  int64_t len, per_slice;
  l.wb = erpl_cmp_block_words(N, P);
  l.chunks = erpl_cmp_chunks(N, l.wb, &len);
  l.slices = erpl_cmp_slices(N, l.wb, &per_slice);
  const size_t cols = (size_t)l.wb * 64, all = (size_t)l.words * 64, tiles = (uN + ERPL_CMP_TILE - 1) / ERPL_CMP_TILE;
  ErplCarve d;
  for (int j = 0; j < R; ++j) l.val[j] = d.take(8 * uN);
  l.xy = d.take(bivariate ? 16 * uN : 0);
  l.keys = d.take(16 * uN);
  l.idx = d.take(8 * uN);
  l.temp_bytes = erpl_scratch_piece(sort_bytes);
  l.temp = d.take(l.temp_bytes);
  for (int j = 0; j < R; ++j) l.sidx[j] = d.take(4 * uN);
  for (int j = 0; j < R; ++j) l.r2e[j] = d.take(8 * uN);
  l.thr = d.take(16 * all);
  l.bits = d.take(8 * uN * (size_t)l.wb);
  l.cnt = d.take(4 * (size_t)l.chunks * cols);
  l.part = d.take(64 * (size_t)l.chunks * cols);
  l.rank = d.take(64 * uR * all);
  l.at_value = d.take(8 * uR);
  l.epart = d.take(bivariate ? 8 * 3 * cols * tiles * (size_t)l.slices : 0);
  l.eout = d.take(8 * 3 * all);
  l.need = d.end;
  return l;
}

// erpl_mc_reweight over n columns: [work: the partials of the workgroups, the state of the selection and the sums handed back,
// work_bytes of them (the struct is erpl_reweight.hip's)][logw n doubles unless the caller keeps them][weights n int64 unless
// the caller keeps them]
struct ErplRwLayout { size_t work, logw, weights, need; };
inline ErplRwLayout erpl_rw_layout(int64_t n, bool caller_keeps_logw, bool caller_keeps_weights, size_t work_bytes) {
  const size_t un = (size_t)n;
  ErplCarve c;
  ErplRwLayout l = {};
  l.work = c.take(work_bytes);
  l.logw = c.take(caller_keeps_logw ? 0 : 8 * un);
  l.weights = c.take(caller_keeps_weights ? 0 : 8 * un);
  l.need = c.end;
  return l;
}

// erpl_mc_corridor_drivers over m columns, R rows, F factors.  The shapes of its passes are functions of m (and of F and
// `regression` for the widths) alone, never of R: a row's results do not depend on which other rows are in the call.
#define ERPL_CDRV_TILE_ROWS 32          // rows of `values` per workgroup of the product pass: two 16-row blocks of memberships, two of y'
#define ERPL_CDRV_KT 16                 // members per LDS stage of the product pass
#define ERPL_CDRV_LIN 48                // the linear columns of a row: x'_0 .. x'_31, the ones at 32, zeros behind them
#define ERPL_CDRV_ONE 32
#define ERPL_CDRV_ZERO 33
#define ERPL_CDRV_SEG 65536             // columns a segment of the moment passes has at the least
#define ERPL_CDRV_MAX_SEGS 64
#define ERPL_CDRV_SLICE 4096            // members a slice of the product pass has at the least
#define ERPL_CDRV_MAX_SLICES 32
#define ERPL_CDRV_PART_BYTES ((size_t)256 << 20)   // the partial tiles of one launch of the product pass
// segments of the moment passes; *seg_len: columns per segment, a multiple of 256
inline int erpl_cdrv_segments(int64_t m, int64_t* seg_len) {
  int64_t s = (m + ERPL_CDRV_SEG - 1) / ERPL_CDRV_SEG;
  if (s > ERPL_CDRV_MAX_SEGS) s = ERPL_CDRV_MAX_SEGS;
  const int64_t per = ((m + s - 1) / s + 255) / 256 * 256;
  *seg_len = per;
  return (int)((m + per - 1) / per);
}
// slices of the product pass; *slice_len: members per slice, a multiple of ERPL_CDRV_KT
inline int erpl_cdrv_slices(int64_t m, int64_t* slice_len) {
  int64_t s = (m + ERPL_CDRV_SLICE - 1) / ERPL_CDRV_SLICE;
  if (s > ERPL_CDRV_MAX_SLICES) s = ERPL_CDRV_MAX_SLICES;
  const int64_t per = ((m + s - 1) / s + ERPL_CDRV_KT - 1) / ERPL_CDRV_KT * ERPL_CDRV_KT;
  *slice_len = per;
  return (int)((m + per - 1) / per);
}
// the product columns x'_f x'_g a row carries: the F squares first, then - with the regression - the pairs f < g row by row
inline int erpl_cdrv_products(int F, bool regression) { return regression ? F * (F + 1) / 2 : F; }
inline int erpl_cdrv_product_index(int F, int f, int g) { return f == g ? f : F + f * (2 * F - f - 1) / 2 + (g - f - 1); }
inline int erpl_cdrv_product_blocks(int F, bool regression) { return (erpl_cdrv_products(F, regression) + 15) / 16; }
// doubles of a row of sums: [memberships x linear columns 48][memberships x products, whole blocks of 16][y' x linear columns 48]
// [sum y'^2][padding to a multiple of 4]
inline int erpl_cdrv_row_doubles(int F, bool regression) {
  return (2 * ERPL_CDRV_LIN + 16 * erpl_cdrv_product_blocks(F, regression) + 1 + 3) / 4 * 4;
}
// tiles of ERPL_CDRV_TILE_ROWS rows one launch of the product pass takes: what fits ERPL_CDRV_PART_BYTES, at least one
inline int erpl_cdrv_chunk_tiles(int64_t m, int F, bool regression) {
  int64_t len;
  const size_t tile = 8 * (size_t)ERPL_CDRV_TILE_ROWS * (size_t)erpl_cdrv_row_doubles(F, regression) * (size_t)erpl_cdrv_slices(m, &len);
  const size_t t = ERPL_CDRV_PART_BYTES / tile;
  return (int)(t < 1 ? 1 : t);
}
// [base m bytes][counts 4 u64][fstat F records of 8 doubles][rstat R records of 8 doubles][mpart max(F, R) segs 4 doubles: the
// partials of a moment pass][part chunk_tiles slices tiles of 32 rows of row_doubles][sums chunk_tiles 32 rows of row_doubles]
// [pairs R F (row, factor) int32 pairs: the pairs whose extremes are asked for][ext R F (min, max)]
struct ErplCdrvLayout {
  size_t base, count, fstat, rstat, mpart, part, sums, pairs, ext, need;
  int64_t seg_len, slice_len;
  int segs, slices, chunk_tiles, row_doubles;
};
inline ErplCdrvLayout erpl_cdrv_layout(int64_t m, int R, int F, bool regression) {
  const size_t um = (size_t)m, uR = (size_t)R, uF = (size_t)F;
  ErplCarve c;
  ErplCdrvLayout l = {};
  l.segs = erpl_cdrv_segments(m, &l.seg_len);
  l.slices = erpl_cdrv_slices(m, &l.slice_len);
  l.row_doubles = erpl_cdrv_row_doubles(F, regression);
  l.chunk_tiles = erpl_cdrv_chunk_tiles(m, F, regression);
  const size_t tiles = (uR + ERPL_CDRV_TILE_ROWS - 1) / ERPL_CDRV_TILE_ROWS;
  const size_t chunk = tiles < (size_t)l.chunk_tiles ? tiles : (size_t)l.chunk_tiles;
  const size_t tile_bytes = 8 * (size_t)ERPL_CDRV_TILE_ROWS * (size_t)l.row_doubles;
  l.base = c.take(um);
  l.count = c.take(32);
  l.fstat = c.take(64 * uF);
  l.rstat = c.take(64 * uR);
  l.mpart = c.take(32 * (uR > uF ? uR : uF) * (size_t)l.segs);
  l.part = c.take(tile_bytes * chunk * (size_t)l.slices);
  l.sums = c.take(tile_bytes * chunk);
  l.pairs = c.take(8 * uR * uF);
  l.ext = c.take(16 * uR * uF);
  l.need = c.end;
  return l;
}
