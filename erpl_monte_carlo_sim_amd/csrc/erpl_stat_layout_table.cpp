// erpl_stat_layout_table.cpp — prints what erpl_stat_layout.h lays out, for tests/test_stat_layout.py (host compiler only,
// no HIP).  stdin, one request per line; stdout, one line per request: the offsets in the order of the struct, then the
// scratch size the launches are told and `need`.
//   corr <n> <V> <ranks> <caller_keeps_ranks> <temp_bytes>               -> keys ranks idx temp pop temp_bytes need
//   boot <n> <R> <n_stats> <B> <caller_keeps_replicates> <temp_bytes>    -> pop src count x[R] sorted[R] pos[R] keys idx temp zero
//                                                                           rep temp_bytes need
//   dens <n> <nodes> <want_samples> <caller_keeps_row> <temp_bytes>      -> pop src count temp pts nodes dens row part temp_bytes need
//   sobol <n> <k> <R> <B> <caller_keeps_replicates> <temp_bytes>         -> pop src[R] count rec[R] temp rep temp_bytes need
//   dep <n> <F> <R> <M> <H> <P> <temp_bytes>                             -> pop src count yd[R] xc yext keys idx temp cstat tab null
//                                                                           x_stride y_stride temp_bytes need
//   cmp <n_a> <n_b> <N> <R> <P> <bivariate> <select_bytes> <sort_bytes>  -> pop_a src_a pop_b src_b count sel_temp sel_bytes pop_need
//                                                                           val[R] xy keys idx temp sidx[R] r2e[R] thr bits cnt part
//                                                                           rank at_value epart eout temp_bytes words wb chunks
//                                                                           slices need
//   sur <n> <R> <P> <temp_bytes>                                         -> pop src count temp model psi part gram yhat temp_bytes
//                                                                           m_kinds m_terms m_coef model_bytes ld slices need
//   surslices <lo> <hi> <P>                                              -> the most slices erpl_sur_slices cuts a chunk of lo .. hi
//                                                                           members into (-1: a chunk its slices do not cover), the
//                                                                           first length that has them, erpl_sur_max_slices(hi, P)
//   surslice <len> <P>                                                   -> slices slice_len of one chunk
//   rw <n> <caller_keeps_logw> <caller_keeps_weights> <work_bytes>       -> work logw weights need
//   wdens <n> <nodes> <want_samples> <caller_keeps_row> <temp_bytes>     -> pop src count temp pts ws nodes dens row part temp_bytes
//                                                                           need
//   cdrv <m> <R> <F> <regression>                                        -> base count fstat rstat mpart part sums pairs ext
//                                                                           seg_len slice_len segs slices chunk_tiles row_doubles
//                                                                           need
#include <stdio.h>

#include <initializer_list>

#include "erpl_stat_layout.h"

static void put(size_t v, const char* end = " ") { printf("%zu%s", v, end); }

int main() {
  char line[256];
  while (fgets(line, sizeof(line), stdin)) {
    long long n, nodes, big;
    int a, b, c, d, e;
    size_t temp, temp2;
    if (sscanf(line, "corr %lld %d %d %d %zu", &n, &a, &b, &c, &temp) == 5) {
      const ErplCorrLayout l = erpl_corr_layout(n, a, b != 0, c != 0, temp);
      for (size_t v : {l.keys, l.ranks, l.idx, l.temp, l.pop, l.temp_bytes}) put(v);
      put(l.need, "\n");
    } else if (sscanf(line, "boot %lld %d %d %d %d %zu", &n, &a, &b, &c, &d, &temp) == 6 && a >= 1 && a <= ERPL_BOOT_MAX_ROWS) {
      const ErplBootLayout l = erpl_boot_layout(n, a, b, c, d != 0, temp);
      for (size_t v : {l.pop, l.src, l.count}) put(v);
      for (const size_t* rows : {l.x, l.sorted, l.pos})
        for (int j = 0; j < a; ++j) put(rows[j]);
      for (size_t v : {l.keys, l.idx, l.temp, l.zero, l.rep, l.temp_bytes}) put(v);
      put(l.need, "\n");
    } else if (sscanf(line, "dens %lld %lld %d %d %zu", &n, &nodes, &a, &b, &temp) == 5) {
      const ErplDensLayout l = erpl_dens_layout(n, nodes, a != 0, b != 0, temp);
      for (size_t v : {l.pop, l.src, l.count, l.temp, l.pts, l.nodes, l.dens, l.row, l.part, l.temp_bytes}) put(v);
      put(l.need, "\n");
    } else if (sscanf(line, "sobol %lld %d %d %d %d %zu", &n, &a, &b, &c, &d, &temp) == 6 && b >= 1 && b <= ERPL_SOBOL_MAX_ROWS) {
      const ErplSobolLayout l = erpl_sobol_layout(n, a, b, c, d != 0, temp);
      put(l.pop);
      for (int j = 0; j < b; ++j) put(l.src[j]);
      put(l.count);
      for (int j = 0; j < b; ++j) put(l.rec[j]);
      for (size_t v : {l.temp, l.rep, l.temp_bytes}) put(v);
      put(l.need, "\n");
    } else if (sscanf(line, "dep %lld %d %d %d %d %d %zu", &n, &a, &b, &c, &d, &e, &temp) == 7 && b >= 1 && b <= ERPL_DEP_MAX_ROWS) {
      const ErplDepLayout l = erpl_dep_layout(n, a, b, c, d, e, temp);
      for (size_t v : {l.pop, l.src, l.count}) put(v);
      for (int j = 0; j < b; ++j) put(l.yd[j]);
      for (size_t v : {l.xc, l.yext, l.keys, l.idx, l.temp, l.cstat, l.tab, l.null, l.x_stride, l.y_stride, l.temp_bytes}) put(v);
      put(l.need, "\n");
    } else if (sscanf(line, "cmp %lld %lld %lld %d %d %d %zu %zu", &n, &nodes, &big, &a, &b, &c, &temp, &temp2) == 8 && a >= 1 &&
               a <= ERPL_CMP_MAX_ROWS) {
      const ErplCompareLayout l = erpl_compare_layout(n, nodes, big, a, b, c != 0, temp, temp2);
      for (size_t v : {l.pop_a, l.src_a, l.pop_b, l.src_b, l.count, l.sel_temp, l.sel_bytes, l.pop_need}) put(v);
      for (int j = 0; j < a; ++j) put(l.val[j]);
      for (size_t v : {l.xy, l.keys, l.idx, l.temp}) put(v);
      for (const size_t* rows : {l.sidx, l.r2e})
        for (int j = 0; j < a; ++j) put(rows[j]);
      for (size_t v : {l.thr, l.bits, l.cnt, l.part, l.rank, l.at_value, l.epart, l.eout, l.temp_bytes}) put(v);
      for (int v : {l.words, l.wb, l.chunks, l.slices}) put((size_t)v);
      put(l.need, "\n");
    } else if (sscanf(line, "sur %lld %d %d %zu", &n, &a, &b, &temp) == 4 && a >= 1 && a <= ERPL_SUR_MAX_ROWS) {
      const ErplSurLayout l = erpl_sur_layout(n, a, b, temp);
      for (size_t v : {l.pop, l.src, l.count, l.temp, l.model, l.psi, l.part, l.gram, l.yhat, l.temp_bytes, l.m_kinds, l.m_terms, l.m_coef,
                       l.model_bytes, (size_t)l.ld, (size_t)l.slices})
        put(v);
      put(l.need, "\n");
    } else if (sscanf(line, "surslices %lld %lld %d", &n, &nodes, &a) == 3 && n >= 1 && nodes >= n) {
      // every chunk length from <lo> to <hi>: the most slices any of them is cut into, and the first length that has them
      int most = 0, len = 0;
      long long at = n;
      for (long long k = n; k <= nodes; ++k) {
        const int s = erpl_sur_slices(k, a, &len);
        if (s > most) { most = s; at = k; }
        if ((long long)s * len < k || len % ERPL_SUR_KT != 0) { most = -1; at = k; break; }   // the slices do not cover the chunk
      }
      printf("%d %lld %d\n", most, at, erpl_sur_max_slices(nodes, a));
    } else if (sscanf(line, "surslice %lld %d", &n, &a) == 2 && n >= 1) {
      int len = 0;
      const int s = erpl_sur_slices(n, a, &len);
      printf("%d %d\n", s, len);
    } else if (sscanf(line, "rw %lld %d %d %zu", &n, &a, &b, &temp) == 4) {
      const ErplRwLayout l = erpl_rw_layout(n, a != 0, b != 0, temp);
      for (size_t v : {l.work, l.logw, l.weights}) put(v);
      put(l.need, "\n");
    } else if (sscanf(line, "wdens %lld %lld %d %d %zu", &n, &nodes, &a, &b, &temp) == 5) {
      const ErplDensWLayout l = erpl_densw_layout(n, nodes, a != 0, b != 0, temp);
      for (size_t v : {l.pop, l.src, l.count, l.temp, l.pts, l.ws, l.nodes, l.dens, l.row, l.part, l.temp_bytes}) put(v);
      put(l.need, "\n");
    } else if (sscanf(line, "cdrv %lld %d %d %d", &n, &a, &b, &c) == 4 && n >= 1 && a >= 1 && b >= 1 && b <= ERPL_CDRV_MAX_FACTORS) {
      const ErplCdrvLayout l = erpl_cdrv_layout(n, a, b, c != 0);
      for (size_t v : {l.base, l.count, l.fstat, l.rstat, l.mpart, l.part, l.sums, l.pairs, l.ext, (size_t)l.seg_len, (size_t)l.slice_len,
                       (size_t)l.segs, (size_t)l.slices, (size_t)l.chunk_tiles, (size_t)l.row_doubles})
        put(v);
      put(l.need, "\n");
    } else {
      fprintf(stderr, "bad request: %s", line);
      return 1;
    }
  }
  return 0;
}
