// erpl_stats_api.hip — host halves of the analysis entry points of the C ABI (include/erpl_mc.h): erpl_mc_analyze,
// erpl_mc_histogram, erpl_mc_histogram_xy, erpl_mc_dispersion, erpl_mc_correlation, erpl_mc_bootstrap, erpl_mc_impact_density,
// erpl_mc_impact_density_weighted,
// erpl_mc_corridor_resample, erpl_mc_corridor_bands, erpl_mc_corridor_depth, erpl_mc_sobol, erpl_mc_dependence, erpl_mc_compare and their defaults.
// Argument checks, workspace, launches (erpl_analysis.hip, erpl_distributions.hip, erpl_correlation.hip, erpl_bootstrap.hip,
// erpl_density.hip, erpl_density_w.hip, erpl_corridor.hip, erpl_corridor_depth.hip, erpl_sobol.hip, erpl_dependence.hip, erpl_compare.hip)
// and what the host finishes in double precision.  The refusals come in one order
// everywhere - spec fields, n, pointers, context (erpl_mc_bootstrap: the order its header comment lists) - and need no
// device; tests/golden/stats_refusals.json pins their texts.  What the entry points share comes first: the pieces of the
// argument checks, describe_rows, the host finish of a described row and of a landing cloud.  The growing buffers are laid
// out in erpl_stat_layout.h; the context keeps an ErplStatUnit per unit (erpl_host.h).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "erpl_cdrv.h"
#include "erpl_depth.h"
#include "erpl_host.h"
#include "erpl_philox.h"
#include "erpl_reweight.h"
#include "erpl_tally.h"

namespace {

// a pointer the call needs, refused by the name of the argument
#define NEED_AS(p, name) do { if (!(p)) return erpl_fail(ERPL_ERR_INVALID, name " is NULL"); } while (0)
#define NEED(p) NEED_AS(p, #p)

// an integer field of a spec in lo..hi; j >= 0: element j of an array field
int check_int(int v, const char* name, int j, int lo, int hi) {
  if (v >= lo && v <= hi) return ERPL_OK;
  if (j >= 0) return erpl_fail(ERPL_ERR_INVALID, "spec->%s[%d] = %d outside %d..%d", name, j, v, lo, hi);
  return erpl_fail(ERPL_ERR_INVALID, "spec->%s = %d outside %d..%d", name, v, lo, hi);
}

// n_rows in lo..hi, then spec->rows of any spec: rows in 0..last, none listed twice
int check_row_list(const int32_t* rows, int n_rows, int lo, int hi, int last = ERPL_SUMMARY_DIM - 1) {
  ERPL_TRY(check_int(n_rows, "n_rows", -1, lo, hi));
  for (int j = 0; j < n_rows; ++j) {
    ERPL_TRY(check_int(rows[j], "rows", j, 0, last));
    for (int k = 0; k < j; ++k)
      if (rows[k] == rows[j]) return erpl_fail(ERPL_ERR_INVALID, "spec->rows[%d] = %d is listed twice", j, rows[j]);
  }
  return ERPL_OK;
}

// row_x / row_y of a spec about the landing plane: two different summary rows
int check_row_pair(int row_x, int row_y) {
  ERPL_TRY(check_int(row_x, "row_x", -1, 0, ERPL_SUMMARY_DIM - 1));
  ERPL_TRY(check_int(row_y, "row_y", -1, 0, ERPL_SUMMARY_DIM - 1));
  if (row_x == row_y) return erpl_fail(ERPL_ERR_INVALID, "spec->row_y = %d is listed twice (row_x)", row_y);
  return ERPL_OK;
}

// spec->q of any spec: at most ERPL_ANALYSIS_MAX_Q fractions in [0, 1]
int check_quantiles(const double* q, int n_q) {
  ERPL_TRY(check_int(n_q, "n_q", -1, 0, ERPL_ANALYSIS_MAX_Q));
  for (int j = 0; j < n_q; ++j)
    if (!(q[j] >= 0.0 && q[j] <= 1.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->q[%d] = %g outside [0, 1]", j, q[j]);
  return ERPL_OK;
}

// spec->level of erpl_dispersion_spec and erpl_density_spec: at most `most` contents in (0, 1)
int check_levels(const double* level, int n_levels, int most) {
  ERPL_TRY(check_int(n_levels, "n_levels", -1, 0, most));
  for (int k = 0; k < n_levels; ++k)
    if (!(level[k] > 0.0 && level[k] < 1.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->level[%d] = %g outside (0, 1)", k, level[k]);
  return ERPL_OK;
}

// n: at least one sample and, where sample indices are carried in fewer bits, at most `most` (`why` ends the refusal)
int check_n(int64_t n, int64_t most = INT64_MAX, const char* why = "") {
  if (n <= 0) return erpl_fail(ERPL_ERR_INVALID, "n = %lld: need at least one sample", (long long)n);
  if (n > most) return erpl_fail(ERPL_ERR_INVALID, "n = %lld%s", (long long)n, why);
  return ERPL_OK;
}

// Rows of `summary` ([.][n]; rows == NULL: its first n_rows rows) through the moment passes and the selection of
// erpl_mc_analyze with `why` as the mask (read only there), and the copy of what they find into the pinned `out`.
int describe_rows(erpl_ctx* c, const double* summary, const uint8_t* why, int64_t n, const int32_t* rows, int n_rows,
                  const double* q, int n_q, ErplAnaResult* out, hipStream_t st) {
  ErplAnaArgs a;
  memset(&a, 0, sizeof(a));
  a.summary = summary; a.why = const_cast<uint8_t*>(why); a.work = c->ana.work; a.n = n; a.n_rows = n_rows; a.n_q = n_q;
  for (int j = 0; j < n_rows; ++j) a.rows[j] = rows ? rows[j] : j;
  for (int k = 0; k < n_q; ++k) a.q[k] = q[k];
  KERNEL_TRY(erpl_launch_row_stats(a, st));
  HIP_TRY(hipMemcpyAsync(out, &c->ana.work->res, sizeof(ErplAnaResult), hipMemcpyDeviceToHost, st));
  return ERPL_OK;
}

// count, mean and covariance of a landing cloud into a result that has these fields: NaN when nothing was counted
template <typename Result>
bool finish_cloud(Result* r, unsigned long long count, double mean_x, double mean_y, double cov_xx, double cov_xy, double cov_yy) {
  const bool any = count > 0ull;
  const double nan = NAN;
  r->count = (int64_t)count;
  r->mean_x = any ? mean_x : nan; r->mean_y = any ? mean_y : nan;
  r->cov_xx = any ? cov_xx : nan; r->cov_xy = any ? cov_xy : nan; r->cov_yy = any ? cov_yy : nan;
  return any;
}

// the inverse of key_of_signed (erpl_stat_device.h)
double double_of_key(unsigned long long k) {
  const unsigned long long b = k ^ ((k >> 63) ? (1ull << 63) : ~0ull);
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}

// What the host finishes of one described row: the population std from m2, the order statistics back from their sort keys
// and the linear interpolation between them.  A row that is not described, or has no finite valid value, is all NaN.
void finish_row_stats(const ErplAnaRow& r, const double* q, int n_q, bool described, erpl_row_stats& o) {
  const double nan = NAN;
  o.count = described ? (int64_t)r.count : 0;
  const bool any = described && r.count > 0ull;
  const double cnt = (double)r.count;
  o.mean = any ? r.mean : nan;
  o.std = any ? sqrt(r.m2 / cnt) : nan;
  o.min = any ? r.vmin : nan;
  o.max = any ? r.vmax : nan;
  for (int k = 0; k < ERPL_ANALYSIS_MAX_Q; ++k) {
    if (!any || k >= n_q) { o.quantile[k] = o.order_lo[k] = o.order_hi[k] = nan; continue; }
    const double pos = q[k] * (double)(r.count - 1ull);   // as on the device, which chose the ranks from it
    const double lo = floor(pos);
    o.order_lo[k] = double_of_key(r.key[2 * k]);
    o.order_hi[k] = double_of_key(r.key[2 * k + 1]);
    o.quantile[k] = o.order_lo[k] + (o.order_hi[k] - o.order_lo[k]) * (pos - lo);
  }
}

int check_analysis_spec(const erpl_analysis_spec* s) {
  const double bound[5] = {s->max_apogee, s->min_apogee, s->max_range, s->max_flight_time, s->energy_apogee};
  const char* name[5] = {"max_apogee", "min_apogee", "max_range", "max_flight_time", "energy_apogee"};
  for (int k = 0; k < 5; ++k)
    if (std::isnan(bound[k])) return erpl_fail(ERPL_ERR_INVALID, "spec->%s is NaN", name[k]);
  ERPL_TRY(check_row_list(s->rows, s->n_rows, 0, ERPL_ANALYSIS_MAX_ROWS));
  return check_quantiles(s->q, s->n_q);
}

}  // namespace

extern "C" {

int erpl_mc_analysis_defaults(erpl_analysis_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->max_apogee = 80000.0;        // monte_carlo.py:343-346
  spec->min_apogee = 100.0;
  spec->max_range = 200000.0;
  spec->max_flight_time = 600.0;
  const double v_max = 1200.0, g = 9.81;
  const double h_max = v_max * v_max / (2 * g);   // monte_carlo.py:349-353: theoretical_max_altitude, then * 1.2
  spec->energy_apogee = h_max * 1.2;
  spec->n_rows = 3;
  spec->rows[0] = ERPL_SUM_APOGEE_ALT; spec->rows[1] = ERPL_SUM_RANGE; spec->rows[2] = ERPL_SUM_FLIGHT_TIME;
  spec->n_q = 5;
  const double q[5] = {0.05, 0.25, 0.5, 0.75, 0.95};
  for (int j = 0; j < 5; ++j) spec->q[j] = q[j];
  return ERPL_OK;
}

int erpl_mc_analyze(erpl_ctx* c, const double* summary, const int32_t* status, int64_t n, const erpl_analysis_spec* spec,
                    erpl_analysis* result, uint8_t* reasons, void* stream) {
  // spec, n and the pointers before the context: the argument checks need no device
  NEED(spec);
  ERPL_TRY(check_analysis_spec(spec));
  ERPL_TRY(check_n(n));
  NEED(summary); NEED(result); NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  ERPL_TRY(c->ana.first_use());
  ERPL_TRY(c->ana.grow((size_t)n));   // one reason byte per sample
  ErplAnaArgs a;
  memset(&a, 0, sizeof(a));
  a.summary = summary; a.status = status; a.why = (uint8_t*)c->ana.buf; a.reasons = reasons; a.work = c->ana.work; a.n = n;
  a.max_apogee = spec->max_apogee; a.min_apogee = spec->min_apogee; a.max_range = spec->max_range;
  a.max_flight_time = spec->max_flight_time; a.energy_apogee = spec->energy_apogee;
  a.n_rows = spec->n_rows; a.n_q = spec->n_q;
  for (int j = 0; j < spec->n_rows; ++j) a.rows[j] = spec->rows[j];
  for (int j = 0; j < spec->n_q; ++j) a.q[j] = spec->q[j];
  KERNEL_TRY(erpl_launch_analysis(a, stream));
  HIP_TRY(hipMemcpyAsync(c->ana.host, &c->ana.work->res, sizeof(ErplAnaResult), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));

  const ErplAnaResult& d = *c->ana.host;
  memset(result, 0, sizeof(*result));
  result->n = n;
  result->n_valid = (int64_t)d.counter[13];
  result->n_outliers = n - result->n_valid;
  for (int k = 0; k < 6; ++k) result->reason_counts[k] = (int64_t)d.counter[k];
  for (int k = 0; k < 5; ++k) result->termination_counts[k] = (int64_t)d.counter[6 + k];
  result->n_status_nan = (int64_t)d.counter[11];
  result->n_incomplete = (int64_t)d.counter[12];
  for (int j = 0; j < ERPL_ANALYSIS_MAX_ROWS; ++j) finish_row_stats(d.row[j], spec->q, spec->n_q, j < spec->n_rows, result->row[j]);
  if (result->n_incomplete > 0)
    return erpl_fail(ERPL_ERR_INCOMPLETE, "%lld sample(s) carry ERPL_ST_INCOMPLETE: they were never integrated",
                (long long)result->n_incomplete);
  return ERPL_OK;
}

}  // extern "C"

// ------------------------------------------------- erpl_mc_histogram, erpl_mc_histogram_xy, erpl_mc_dispersion
namespace {

// lo / hi of one axis as the caller gave them: 1 = from the data, 0 = explicit, < 0 = refused
int check_range(double lo, double hi, const char* lo_name, const char* hi_name, int j) {
  char at[16] = "";
  if (j >= 0) snprintf(at, sizeof(at), "[%d]", j);
  if (std::isnan(lo) && std::isnan(hi)) return 1;
  if (std::isnan(lo) || std::isnan(hi))
    return erpl_fail(ERPL_ERR_INVALID, "spec->%s%s = %g, spec->%s%s = %g: both NaN (range from the data) or both finite", lo_name, at,
                lo, hi_name, at, hi);
  if (!std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(hi - lo))
    return erpl_fail(ERPL_ERR_INVALID, "spec->%s%s = %g, spec->%s%s = %g: not a finite range", lo_name, at, lo, hi_name, at, hi);
  if (lo > hi) return erpl_fail(ERPL_ERR_INVALID, "spec->%s%s = %g > spec->%s%s = %g", lo_name, at, lo, hi_name, at, hi);
  return 0;
}

// The range in use: min / max found on the device for an automatic one ((0, 1) if nothing was counted), widened by a
// half either side if empty.  false: hi - lo is not finite.
bool settle_range(bool automatic, double found_lo, double found_hi, double* lo, double* hi) {
  if (automatic) {
    if (found_lo > found_hi) { found_lo = 0.0; found_hi = 1.0; }
    *lo = found_lo; *hi = found_hi;
  }
  if (!std::isfinite(*hi - *lo)) return false;
  if (*lo == *hi) { *lo -= 0.5; *hi += 0.5; }
  return true;
}

// np.linspace(lo, hi, bins + 1): two roundings per edge (this file is compiled without contraction), the last edge exact
// (the edge rule is ErplEdges of erpl_tally.h: the tally computes the same edges on the device)
void fill_edges(double lo, double hi, int bins, double* e) {
  const ErplEdges edge = erpl_edges_of(lo, hi, bins);
  for (int i = 0; i <= bins; ++i) e[i] = edge[i];
}

// A histogram call from "args filled" to "edges on the device": the range pass if some axis is automatic, the range in use
// and the np.linspace edges of every axis in the pinned mirror, and their upload.  too_wide(j): the caller's refusal of an
// axis whose range is wider than a double holds - the entry points name their fields differently.
template <typename Refuse>
int dist_edges(erpl_ctx* c, ErplDistArgs& a, hipStream_t st, Refuse too_wide) {
  DistHost& h = *c->dist.host;
  bool any_auto = false;
  for (int j = 0; j < a.n_rows; ++j) any_auto = any_auto || a.automatic[j] != 0;
  if (any_auto) {
    KERNEL_TRY(erpl_launch_dist_range(a, st));
    HIP_TRY(hipMemcpyAsync(&h.range, &c->dist.work->range, sizeof(ErplDistRange), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  memset(h.edges, 0, (size_t)a.n_rows * sizeof(h.edges[0]));
  for (int j = 0; j < a.n_rows; ++j) {
    if (!settle_range(a.automatic[j] != 0, h.range.lo[j], h.range.hi[j], &a.lo[j], &a.hi[j])) return too_wide(j);
    fill_edges(a.lo[j], a.hi[j], a.bins[j], h.edges[j]);
  }
  HIP_TRY(hipMemcpyAsync(&c->dist.work->edges[0][0], &h.edges[0][0], (size_t)a.n_rows * sizeof(h.edges[0]),
                         hipMemcpyHostToDevice, st));
  return ERPL_OK;
}

}  // namespace

extern "C" {

int erpl_mc_histogram_defaults(erpl_hist_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->n_rows = 3;
  spec->rows[0] = ERPL_SUM_APOGEE_ALT; spec->rows[1] = ERPL_SUM_RANGE; spec->rows[2] = ERPL_SUM_FLIGHT_TIME;
  for (int j = 0; j < ERPL_HIST_MAX_ROWS; ++j) { spec->bins[j] = 50; spec->lo[j] = spec->hi[j] = NAN; }   // monte_carlo.py:570
  return ERPL_OK;
}

int erpl_mc_histogram(erpl_ctx* c, const double* summary, const uint8_t* mask, int64_t n, const erpl_hist_spec* spec,
                      double* edges, int64_t* counts, erpl_hist_result* result, void* stream) {
  NEED(spec);
  ERPL_TRY(check_row_list(spec->rows, spec->n_rows, 1, ERPL_HIST_MAX_ROWS));
  ErplDistArgs a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < spec->n_rows; ++j) {
    ERPL_TRY(check_int(spec->bins[j], "bins", j, 1, ERPL_HIST_MAX_BINS));
    const int rc = check_range(spec->lo[j], spec->hi[j], "lo", "hi", j);
    if (rc < 0) return rc;
    a.rows[j] = spec->rows[j]; a.partner[j] = -1; a.bins[j] = spec->bins[j]; a.automatic[j] = rc;
    a.lo[j] = spec->lo[j]; a.hi[j] = spec->hi[j];
  }
  ERPL_TRY(check_n(n));
  NEED(summary); NEED(edges); NEED(counts); NEED(result); NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  ERPL_TRY(c->dist.first_use());
  hipStream_t st = (hipStream_t)stream;
  DistHost& h = *c->dist.host;
  a.summary = summary; a.mask = mask; a.work = c->dist.work; a.n = n; a.n_rows = spec->n_rows;
  ERPL_TRY(dist_edges(c, a, st, [&](int j) {
    return erpl_fail(ERPL_ERR_INVALID, "spec->rows[%d] = %d: the range of the counted values, %g to %g, is wider than a double holds",
                     j, spec->rows[j], a.lo[j], a.hi[j]);
  }));
  KERNEL_TRY(erpl_launch_dist_hist(a, stream));
  HIP_TRY(hipMemcpyAsync(&h.hist, &c->dist.work->hist, sizeof(ErplDistHist), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memset(result, 0, sizeof(*result));
  memcpy(edges, h.edges, (size_t)spec->n_rows * sizeof(h.edges[0]));
  for (int j = 0; j < spec->n_rows; ++j) {
    for (int k = 0; k < ERPL_HIST_MAX_BINS; ++k) counts[(size_t)j * ERPL_HIST_MAX_BINS + k] = (int64_t)h.hist.bins[j][k];
    result->counted[j] = (int64_t)h.hist.counted[j];
    result->below[j] = (int64_t)h.hist.below[j];
    result->above[j] = (int64_t)h.hist.above[j];
    result->lo[j] = a.lo[j]; result->hi[j] = a.hi[j];
  }
  return ERPL_OK;
}

int erpl_mc_histogram_xy(erpl_ctx* c, const double* summary, const uint8_t* mask, int64_t n, const erpl_hist2d_spec* spec,
                        double* edges_x, double* edges_y, int64_t* counts, erpl_hist2d_result* result, void* stream) {
  NEED(spec);
  ERPL_TRY(check_row_pair(spec->row_x, spec->row_y));
  ERPL_TRY(check_int(spec->bins_x, "bins_x", -1, 1, ERPL_HIST2D_MAX_BINS));
  ERPL_TRY(check_int(spec->bins_y, "bins_y", -1, 1, ERPL_HIST2D_MAX_BINS));
  const int auto_x = check_range(spec->lo_x, spec->hi_x, "lo_x", "hi_x", -1);
  if (auto_x < 0) return auto_x;
  const int auto_y = check_range(spec->lo_y, spec->hi_y, "lo_y", "hi_y", -1);
  if (auto_y < 0) return auto_y;
  ERPL_TRY(check_n(n));
  NEED(summary); NEED(edges_x); NEED(edges_y); NEED(counts); NEED(result); NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  ERPL_TRY(c->dist.first_use());
  hipStream_t st = (hipStream_t)stream;
  DistHost& h = *c->dist.host;
  ErplDistArgs a;
  memset(&a, 0, sizeof(a));
  a.summary = summary; a.mask = mask; a.work = c->dist.work; a.n = n; a.n_rows = 2;
  a.rows[0] = spec->row_x; a.rows[1] = spec->row_y; a.partner[0] = spec->row_y; a.partner[1] = spec->row_x;
  a.bins[0] = spec->bins_x; a.bins[1] = spec->bins_y; a.automatic[0] = auto_x; a.automatic[1] = auto_y;
  a.lo[0] = spec->lo_x; a.hi[0] = spec->hi_x; a.lo[1] = spec->lo_y; a.hi[1] = spec->hi_y;
  ERPL_TRY(dist_edges(c, a, st, [&](int j) {
    return erpl_fail(ERPL_ERR_INVALID, "spec->row_%s = %d: the range of the counted values, %g to %g, is wider than a double holds",
                     j ? "y" : "x", a.rows[j], a.lo[j], a.hi[j]);
  }));
  KERNEL_TRY(erpl_launch_dist_hist2d(a, stream));
  const size_t cells = (size_t)spec->bins_x * (size_t)spec->bins_y;
  HIP_TRY(hipMemcpyAsync(&h.counted2, &c->dist.work->counted2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h.cells, c->dist.work->cells, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(edges_x, h.edges[0], (size_t)(spec->bins_x + 1) * sizeof(double));
  memcpy(edges_y, h.edges[1], (size_t)(spec->bins_y + 1) * sizeof(double));
  for (size_t k = 0; k < cells; ++k) counts[k] = (int64_t)h.cells[k];
  memset(result, 0, sizeof(*result));
  result->counted = (int64_t)h.counted2;
  result->outside = (int64_t)h.outside2;
  result->lo_x = a.lo[0]; result->hi_x = a.hi[0]; result->lo_y = a.lo[1]; result->hi_y = a.hi[1];
  return ERPL_OK;
}

int erpl_mc_dispersion_defaults(erpl_dispersion_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->row_x = ERPL_SUM_IMPACT_X; spec->row_y = ERPL_SUM_IMPACT_Y;
  spec->centre = ERPL_CENTRE_POINT;   // the launch site
  spec->n_levels = 3;
  spec->level[0] = 0.5; spec->level[1] = 0.9; spec->level[2] = 0.99;
  spec->n_q = 4;
  spec->q[0] = 0.5; spec->q[1] = 0.9; spec->q[2] = 0.95; spec->q[3] = 0.99;   // quantile[0]: the CEP
  return ERPL_OK;
}

int erpl_mc_dispersion(erpl_ctx* c, const double* summary, const uint8_t* mask, int64_t n, const erpl_dispersion_spec* spec,
                       erpl_dispersion* result, double* miss, void* stream) {
  NEED(spec);
  ERPL_TRY(check_row_pair(spec->row_x, spec->row_y));
  if (spec->centre != ERPL_CENTRE_MEAN && spec->centre != ERPL_CENTRE_POINT)
    return erpl_fail(ERPL_ERR_INVALID, "spec->centre = %d: ERPL_CENTRE_MEAN or ERPL_CENTRE_POINT", spec->centre);
  if (spec->centre == ERPL_CENTRE_POINT && !(std::isfinite(spec->cx) && std::isfinite(spec->cy)))
    return erpl_fail(ERPL_ERR_INVALID, "spec->cx = %g, spec->cy = %g: not a finite point", spec->cx, spec->cy);
  ERPL_TRY(check_levels(spec->level, spec->n_levels, ERPL_DISP_MAX_LEVELS));
  ERPL_TRY(check_quantiles(spec->q, spec->n_q));
  ERPL_TRY(check_n(n));
  NEED(summary); NEED(result); NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  ERPL_TRY(c->dist.first_use());
  if (!miss) ERPL_TRY(c->dist.grow((size_t)n * sizeof(double)));   // the caller keeps no miss distances
  ERPL_TRY(c->ana.first_use());                                     // the selection's block,
  ERPL_TRY(c->ana.grow((size_t)n));                                 // and a row of zero bytes to stand in for a mask
  hipStream_t st = (hipStream_t)stream;
  ErplDispArgs d;
  memset(&d, 0, sizeof(d));
  d.summary = summary; d.mask = mask; d.work = c->dist.work; d.miss = miss ? miss : (double*)c->dist.buf; d.n = n;
  d.row_x = spec->row_x; d.row_y = spec->row_y; d.centre = spec->centre; d.n_levels = spec->n_levels;
  d.cx = spec->cx; d.cy = spec->cy;
  for (int k = 0; k < spec->n_levels; ++k) d.k2[k] = -2.0 * log(1.0 - spec->level[k]);
  KERNEL_TRY(erpl_launch_dispersion(d, stream));
  // the miss distance as a one-row summary through the moment passes and the selection of erpl_mc_analyze
  if (!mask) HIP_TRY(hipMemsetAsync(c->ana.buf, 0, (size_t)n, st));
  ERPL_TRY(describe_rows(c, d.miss, mask ? mask : (const uint8_t*)c->ana.buf, n, nullptr, 1, spec->q, spec->n_q, c->ana.host, st));
  HIP_TRY(hipMemcpyAsync(&c->dist.host->mom, &c->dist.work->mom, sizeof(ErplDistMoments), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  const ErplDistMoments& m = c->dist.host->mom;
  const double nan = NAN;
  memset(result, 0, sizeof(*result));
  const bool any = finish_cloud(result, m.count, m.mean_x, m.mean_y, m.cov_xx, m.cov_xy, m.cov_yy);
  const double half = (m.cov_xx + m.cov_yy) / 2, diff = (m.cov_xx - m.cov_yy) / 2;
  const double root = sqrt(diff * diff + m.cov_xy * m.cov_xy);
  result->var_major = any ? half + root : nan;
  result->var_minor = any ? half - root : nan;
  result->angle = any ? 0.5 * atan2(2 * m.cov_xy, m.cov_xx - m.cov_yy) : nan;
  result->centre_x = any ? m.centre_x : nan; result->centre_y = any ? m.centre_y : nan;
  const bool solid = any && m.det > 0.0 && std::isfinite(m.det);
  for (int k = 0; k < ERPL_DISP_MAX_LEVELS; ++k) {
    const bool asked = k < spec->n_levels;
    result->k2[k] = asked && any ? d.k2[k] : nan;
    // a variance that rounding has taken below zero has no axis: 0, as the degenerate ellipse it is
    result->semi_major[k] = asked && any ? sqrt(d.k2[k] * fmax(result->var_major, 0.0)) : nan;
    result->semi_minor[k] = asked && any ? sqrt(d.k2[k] * fmax(result->var_minor, 0.0)) : nan;
    result->inside[k] = !asked || !any ? 0 : (solid ? (int64_t)m.inside[k] : -1);
  }
  finish_row_stats(c->ana.host->row[0], spec->q, spec->n_q, true, result->miss);
  return ERPL_OK;
}

}  // extern "C"

// ------------------------------------------------- erpl_mc_correlation
namespace {

// S_ab of the blocked upper triangle the device hands back (erpl_tables.h)
double gram_at(const double* g, int nbk, int a, int b) {
  if (a > b) std::swap(a, b);
  const int bi = a / 4, bj = b / 4;
  return g[((bi * (2 * nbk - bi + 1)) / 2 + bj - bi) * 16 + (a % 4) * 4 + (b % 4)];
}

// corr (V x V, row-major) from the centred sums: unit diagonal, NaN where either variable is constant
void corr_from_gram(const double* g, int V, const int32_t* constant, bool any, double* corr) {
  const int nbk = (V + 3) / 4;
  for (int a = 0; a < V; ++a)
    for (int b = 0; b < V; ++b) {
      double r = NAN;
      if (any && !constant[a] && !constant[b])
        r = a == b ? 1.0 : gram_at(g, nbk, a, b) / (sqrt(gram_at(g, nbk, a, a)) * sqrt(gram_at(g, nbk, b, b)));
      corr[(size_t)a * V + b] = r;
    }
}

// (the standardised regression of the rows on the factors is erpl_regress of erpl_cdrv.h: erpl_mc_corridor_drivers shares it)

}  // namespace

extern "C" {

int erpl_mc_correlation_defaults(erpl_corr_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->n_rows = 3;
  spec->rows[0] = ERPL_SUM_APOGEE_ALT; spec->rows[1] = ERPL_SUM_RANGE; spec->rows[2] = ERPL_SUM_FLIGHT_TIME;
  spec->ranks = 1;
  return ERPL_OK;
}

int erpl_mc_correlation(erpl_ctx* c, const double* factors, const double* summary, const uint8_t* mask, int64_t n,
                        const erpl_corr_spec* spec, erpl_corr_result* result, double* corr, double* rank_corr,
                        double* ranks_out, void* stream) {
  NEED(spec);
  ERPL_TRY(check_int(spec->n_factors, "n_factors", -1, 1, ERPL_CORR_MAX_FACTORS));
  ERPL_TRY(check_row_list(spec->rows, spec->n_rows, 1, ERPL_CORR_MAX_ROWS));
  if (spec->ranks != 0 && spec->ranks != 1) return erpl_fail(ERPL_ERR_INVALID, "spec->ranks = %d: 0 or 1", spec->ranks);
  if (!spec->ranks && rank_corr) return erpl_fail(ERPL_ERR_INVALID, "rank_corr is given but spec->ranks = 0");
  if (!spec->ranks && ranks_out) return erpl_fail(ERPL_ERR_INVALID, "ranks_out is given but spec->ranks = 0");
  ERPL_TRY(check_n(n, spec->ranks ? 0xffffffffll : INT64_MAX, " with spec->ranks = 1: the sort carries 32-bit sample indices"));
  NEED(factors); NEED(summary); NEED(result); NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int F = spec->n_factors, R = spec->n_rows, V = F + R;
  const bool ranks = spec->ranks != 0;

  ErplCorrArgs a;
  memset(&a, 0, sizeof(a));
  a.mask = mask; a.n = n; a.n_vars = V;
  size_t temp_bytes = 0;
  if (ranks)
    LAUNCH_TRY(erpl_launch_corr_ranks(a, nullptr, nullptr, nullptr, nullptr, nullptr, &temp_bytes, stream), "radix sort sizing failed");
  const ErplCorrLayout at = erpl_corr_layout(n, V, ranks, ranks_out != nullptr, temp_bytes);
  temp_bytes = at.temp_bytes;
  const size_t un = (size_t)n;
  ERPL_TRY(c->corr.first_use());
  ERPL_TRY(c->corr.grow(at.need));
  char* buf = c->corr.buf;
  a.work = c->corr.work;
  a.pop = (uint8_t*)(buf + at.pop);
  for (int f = 0; f < F; ++f) a.var[f] = factors + (size_t)f * un;
  for (int j = 0; j < R; ++j) a.var[F + j] = summary + (size_t)spec->rows[j] * un;

  KERNEL_TRY(erpl_launch_corr_population(a, stream));
  KERNEL_TRY(erpl_launch_corr_gram(a, 0, stream));
  if (ranks) {
    double* rk = ranks_out ? ranks_out : (double*)(buf + at.ranks);
    for (int v = 0; v < V; ++v)
      LAUNCH_TRY(erpl_launch_corr_ranks(a, a.var[v], rk + (size_t)v * un, (unsigned long long*)(buf + at.keys),
                                        (uint32_t*)(buf + at.idx), buf + at.temp, &temp_bytes, stream),
                 "rank pass failed");
    ErplCorrArgs b = a;
    for (int v = 0; v < V; ++v) b.var[v] = rk + (size_t)v * un;
    KERNEL_TRY(erpl_launch_corr_gram(b, 1, stream));
  }
  HIP_TRY(hipMemcpyAsync(c->corr.host, &c->corr.work->out, sizeof(ErplCorrOut), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  const ErplCorrOut& h = *c->corr.host;
  const double nan = NAN;
  memset(result, 0, sizeof(*result));
  result->n = n;
  result->count = (int64_t)h.counter[0];
  result->n_masked = (int64_t)h.counter[1];
  result->n_non_finite = (int64_t)h.counter[2];
  const bool any = h.counter[0] > 0ull;
  const int nbk = (V + 3) / 4;
  for (int v = 0; v < ERPL_CORR_MAX_VARS; ++v) {
    const bool in = any && v < V;
    result->constant[v] = in && h.vmin[v] == h.vmax[v] ? 1 : 0;
    result->mean[v] = in ? h.mean[v] : nan;
    result->std[v] = in ? sqrt(gram_at(h.gram[0], nbk, v, v) / (double)h.counter[0]) : nan;
    result->min[v] = in ? h.vmin[v] : nan;
    result->max[v] = in ? h.vmax[v] : nan;
  }
  for (int j = 0; j < ERPL_CORR_MAX_ROWS; ++j) {
    for (int f = 0; f < ERPL_CORR_MAX_FACTORS; ++f)
      result->pearson[j][f] = result->spearman[j][f] = result->src[j][f] = result->srrc[j][f] = nan;
    result->r2[j] = result->r2_rank[j] = nan;
  }
  std::vector<double> own((size_t)V * V);
  for (int pass = 0; pass < (ranks ? 2 : 1); ++pass) {
    double* m = pass ? rank_corr : corr;
    if (!m) m = own.data();
    corr_from_gram(h.gram[pass], V, result->constant, any, m);
    double (*rho)[ERPL_CORR_MAX_FACTORS] = pass ? result->spearman : result->pearson;
    for (int j = 0; j < R; ++j)
      for (int f = 0; f < F; ++f) rho[j][f] = m[(size_t)(F + j) * V + f];
    bool ok = false;
    if (any) {
      erpl_corr_result fit;   // filled only if every pivot holds
      for (int j = 0; j < ERPL_CORR_MAX_ROWS; ++j) {
        for (int f = 0; f < ERPL_CORR_MAX_FACTORS; ++f) fit.src[j][f] = nan;
        fit.r2[j] = nan;
      }
      ok = erpl_regress(m, V, F, R, result->constant, fit.src, fit.r2);
      if (ok) {
        memcpy(pass ? result->srrc : result->src, fit.src, sizeof(fit.src));
        memcpy(pass ? result->r2_rank : result->r2, fit.r2, sizeof(fit.r2));
      }
    }
    (pass ? result->rank_regression_ok : result->regression_ok) = ok ? 1 : 0;
  }
  return ERPL_OK;
}

}  // extern "C"

// ------------------------------------------------- erpl_mc_bootstrap
extern "C" {

int erpl_mc_bootstrap_defaults(erpl_boot_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->n_rows = 3;
  spec->rows[0] = ERPL_SUM_APOGEE_ALT; spec->rows[1] = ERPL_SUM_RANGE; spec->rows[2] = ERPL_SUM_FLIGHT_TIME;
  spec->n_q = 5;
  const double q[5] = {0.05, 0.25, 0.5, 0.75, 0.95};   // erpl_mc_analysis_defaults
  for (int j = 0; j < 5; ++j) spec->q[j] = q[j];
  spec->replicates = 2000;
  spec->level = 0.95;
  spec->seed = 0;
  return ERPL_OK;
}

int erpl_mc_bootstrap_indices(uint64_t seed, int64_t replicate, int64_t m, int64_t first, int64_t count, int64_t* out) {
  NEED(out);
  if (m <= 0 || m >= (1ll << 31)) return erpl_fail(ERPL_ERR_INVALID, "m = %lld outside 1..2^31 - 1", (long long)m);
  if (replicate < 0 || replicate > 0xffffffffll)
    return erpl_fail(ERPL_ERR_INVALID, "replicate = %lld outside 0..2^32 - 1", (long long)replicate);
  if (first < 0) return erpl_fail(ERPL_ERR_INVALID, "first = %lld is negative", (long long)first);
  if (count < 0) return erpl_fail(ERPL_ERR_INVALID, "count = %lld is negative", (long long)count);
  if (first > m || count > m - first)
    return erpl_fail(ERPL_ERR_INVALID, "first + count = %lld + %lld is beyond m = %lld", (long long)first, (long long)count,
                     (long long)m);
  for (int64_t t = first; t < first + count;) {
    uint64_t A, B;
    erpl_boot_pair(seed, (uint32_t)replicate, (uint64_t)(t >> 1), &A, &B);
    if ((t & 1) == 0) {
      out[t - first] = (int64_t)erpl_boot_index(A, (uint64_t)m);
      ++t;
      if (t >= first + count) break;
    }
    out[t - first] = (int64_t)erpl_boot_index(B, (uint64_t)m);
    ++t;
  }
  return ERPL_OK;
}

int erpl_mc_bootstrap(erpl_ctx* c, const double* summary, const double* extra, const uint8_t* mask, int64_t n,
                      const erpl_boot_spec* spec, erpl_bootstrap* result, double* replicates_out, void* stream) {
  NEED(spec); NEED(summary); NEED(result);
  ERPL_TRY(check_n(n, (1ll << 31) - 1, ": the draws and the sort carry 31-bit sample indices"));
  ERPL_TRY(check_int(spec->n_rows, "n_rows", -1, 1, ERPL_BOOT_MAX_ROWS));   // the three counts before the contents of rows and q
  ERPL_TRY(check_int(spec->n_q, "n_q", -1, 0, ERPL_ANALYSIS_MAX_Q));
  ERPL_TRY(check_int(spec->replicates, "replicates", -1, 1, ERPL_BOOT_MAX_REPLICATES));
  ERPL_TRY(check_row_list(spec->rows, spec->n_rows, 1, ERPL_BOOT_MAX_ROWS, ERPL_BOOT_ROW_EXTRA));
  for (int j = 0; j < spec->n_rows; ++j)
    if (spec->rows[j] == ERPL_BOOT_ROW_EXTRA && !extra)
      return erpl_fail(ERPL_ERR_INVALID, "extra is NULL but spec->rows[%d] = %d (ERPL_BOOT_ROW_EXTRA)", j, spec->rows[j]);
  ERPL_TRY(check_quantiles(spec->q, spec->n_q));
  if (!(spec->level > 0.0 && spec->level < 1.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->level = %g outside (0, 1)", spec->level);
  NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int R = spec->n_rows, nq = spec->n_q, ns = 2 + nq, n_stats = R * ns, B = spec->replicates;
  const size_t un = (size_t)n, uB = (size_t)B;

  size_t temp_bytes = 0;
  LAUNCH_TRY(erpl_boot_temp_bytes(n, &temp_bytes), "select / radix sort sizing failed");
  const ErplBootLayout at = erpl_boot_layout(n, R, n_stats, B, replicates_out != nullptr, temp_bytes);
  ERPL_TRY(c->corr.first_use());   // the population pass and its counters
  ERPL_TRY(c->ana.first_use());    // the estimates and the summary over the replicates
  ERPL_TRY(c->boot.first_use());
  ERPL_TRY(c->boot.grow(at.need));
  char* buf = c->boot.buf;
  BootHost& h = *c->boot.host;

  ErplBootPrep p;
  memset(&p, 0, sizeof(p));
  ErplCorrArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.mask = mask; pa.n = n; pa.n_vars = R; pa.work = c->corr.work; pa.pop = (uint8_t*)(buf + at.pop);
  for (int j = 0; j < R; ++j) {
    p.var[j] = spec->rows[j] == ERPL_BOOT_ROW_EXTRA ? extra : summary + (size_t)spec->rows[j] * un;
    pa.var[j] = p.var[j];
    p.x[j] = (double*)(buf + at.x[j]);
    p.sorted[j] = (double*)(buf + at.sorted[j]);
    p.pos[j] = (uint32_t*)(buf + at.pos[j]);
  }
  p.pop = pa.pop; p.src = (uint32_t*)(buf + at.src); p.count = (unsigned long long*)(buf + at.count);
  p.keys = (unsigned long long*)(buf + at.keys); p.idx = (uint32_t*)(buf + at.idx);
  p.temp = buf + at.temp; p.temp_bytes = at.temp_bytes; p.n = n; p.n_rows = R;
  uint8_t* zero = (uint8_t*)(buf + at.zero);
  double* rep = replicates_out ? replicates_out : (double*)(buf + at.rep);

  KERNEL_TRY(erpl_launch_corr_population(pa, stream));
  HIP_TRY(hipMemcpyAsync(h.counter, &c->corr.work->out.counter[0], sizeof(h.counter), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t m = (int64_t)h.counter[0];
  memset(result, 0, sizeof(*result));
  result->n = n; result->count = m; result->n_masked = (int64_t)h.counter[1]; result->n_non_finite = (int64_t)h.counter[2];
  result->n_stats = n_stats; result->replicates = B;
  const double nan = NAN;
  for (int s = 0; s < ERPL_BOOT_MAX_STATS; ++s) {
    erpl_boot_stat& o = result->stat[s];
    o.estimate = o.rep_mean = o.se = o.lo = o.hi = nan;
    o.finite = 0;
  }
  if (m == 0) {
    if (replicates_out) {   // every replicate of an empty population is NaN: the all-ones byte pattern is one
      HIP_TRY(hipMemsetAsync(replicates_out, 0xff, 8 * uB * (size_t)n_stats, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    return ERPL_OK;
  }

  // the estimates, by the passes of erpl_mc_analyze over the n samples with the population bytes as the mask: the summary
  // rows in one launch, `extra` as a one-row summary in a second
  int32_t est_rows[ERPL_BOOT_MAX_ROWS];
  int est_of[ERPL_BOOT_MAX_ROWS], n_est = 0, has_extra = 0;   // row j of the spec: est[0].row[est_of[j]], or est[1].row[0] (-1)
  for (int j = 0; j < R; ++j) {
    if (spec->rows[j] == ERPL_BOOT_ROW_EXTRA) { est_of[j] = -1; has_extra = 1; }
    else { est_of[j] = n_est; est_rows[n_est++] = spec->rows[j]; }
  }
  if (n_est > 0) ERPL_TRY(describe_rows(c, summary, pa.pop, n, est_rows, n_est, spec->q, nq, &h.est[0], st));
  if (has_extra) ERPL_TRY(describe_rows(c, extra, pa.pop, n, nullptr, 1, spec->q, nq, &h.est[1], st));

  // prepare, then the replicates
  p.m = m;
  LAUNCH_TRY(erpl_launch_boot_compact(p, stream), "select failed");
  LAUNCH_TRY(erpl_launch_boot_prepare(p, stream), "prepare failed");
  ErplBootArgs a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < R; ++j) { a.x[j] = p.x[j]; a.sorted[j] = p.sorted[j]; a.pos[j] = p.pos[j]; }
  a.rep = rep; a.seed = spec->seed; a.m = (uint32_t)m; a.n_rows = R; a.n_q = nq; a.replicates = B;
  for (uint64_t top = (uint64_t)m - 1; top; top >>= 8) ++a.n_digits;
  for (int k = 0; k < nq; ++k) {   // the ranks of erpl_ana_finish_first, the same in every replicate
    const double pos = spec->q[k] * (double)(m - 1);
    int64_t lo = (int64_t)floor(pos);
    if (lo > m - 1) lo = m - 1;
    a.rank[2 * k] = (uint32_t)lo;
    a.rank[2 * k + 1] = (uint32_t)(lo + 1 < m ? lo + 1 : m - 1);
    a.frac[k] = pos - floor(pos);
  }
  KERNEL_TRY(erpl_launch_boot_replicates(a, stream));

  // the summary over the replicates: the [n_stats][B] matrix as rows of length B through the same passes, 16 at a time
  const double tail = (1.0 - spec->level) / 2, interval[2] = {tail, 1.0 - tail};
  HIP_TRY(hipMemsetAsync(zero, 0, uB, st));
  for (int first = 0, k = 0; first < n_stats; first += ERPL_ANALYSIS_MAX_ROWS, ++k)
    ERPL_TRY(describe_rows(c, rep + (size_t)first * uB, zero, B, nullptr, std::min(n_stats - first, (int)ERPL_ANALYSIS_MAX_ROWS),
                           interval, 2, &h.sum[k], st));
  HIP_TRY(hipStreamSynchronize(st));

  for (int j = 0; j < R; ++j) {
    erpl_row_stats est;
    finish_row_stats(est_of[j] < 0 ? h.est[1].row[0] : h.est[0].row[est_of[j]], spec->q, nq, true, est);
    for (int k = 0; k < ns; ++k) {
      const int s = j * ns + k;
      erpl_boot_stat& o = result->stat[s];
      o.estimate = k == 0 ? est.mean : k == 1 ? est.std : est.quantile[k - 2];
      const ErplAnaRow& row = h.sum[s / ERPL_ANALYSIS_MAX_ROWS].row[s % ERPL_ANALYSIS_MAX_ROWS];
      erpl_row_stats over;
      finish_row_stats(row, interval, 2, true, over);
      o.finite = over.count;
      // the constant rule of erpl_mc_correlation: a statistic with min == max over its replicates has no spread, whatever
      // sum / count makes of that value
      const bool constant = over.count > 0 && row.vmin == row.vmax;
      o.rep_mean = constant ? row.vmin : over.mean;
      o.se = over.count == 0 ? nan : (constant ? 0.0 : sqrt(row.m2 / (double)(over.count - 1)));
      o.lo = over.quantile[0];
      o.hi = over.quantile[1];
    }
  }
  return ERPL_OK;
}

}  // extern "C"

// ------------------------------------------------- erpl_mc_impact_density
namespace {

// one axis of erpl_density_spec: 1 = from the data, 0 = explicit with lo < hi, < 0 = refused
int check_density_range(double lo, double hi, const char* lo_name, const char* hi_name) {
  const int rc = check_range(lo, hi, lo_name, hi_name, -1);
  if (rc == 0 && !(lo < hi)) return erpl_fail(ERPL_ERR_INVALID, "spec->%s = %g >= spec->%s = %g", lo_name, lo, hi_name, hi);
  return rc;
}

int check_density_spec(const erpl_density_spec* s) {
  ERPL_TRY(check_row_pair(s->row_x, s->row_y));
  ERPL_TRY(check_int(s->nodes_x, "nodes_x", -1, 2, ERPL_DENSITY_MAX_NODES));
  ERPL_TRY(check_int(s->nodes_y, "nodes_y", -1, 2, ERPL_DENSITY_MAX_NODES));
  if (check_density_range(s->lo_x, s->hi_x, "lo_x", "hi_x") < 0) return ERPL_ERR_INVALID;
  if (check_density_range(s->lo_y, s->hi_y, "lo_y", "hi_y") < 0) return ERPL_ERR_INVALID;
  if (!(std::isfinite(s->pad) && s->pad >= 0.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->pad = %g: finite and >= 0", s->pad);
  if (s->bandwidth != ERPL_BW_SCOTT && s->bandwidth != ERPL_BW_MATRIX)
    return erpl_fail(ERPL_ERR_INVALID, "spec->bandwidth = %d: ERPL_BW_SCOTT or ERPL_BW_MATRIX", s->bandwidth);
  if (s->bandwidth == ERPL_BW_SCOTT && !(std::isfinite(s->bw_scale) && s->bw_scale > 0.0))
    return erpl_fail(ERPL_ERR_INVALID, "spec->bw_scale = %g: finite and > 0", s->bw_scale);
  if (s->bandwidth == ERPL_BW_MATRIX) {
    const bool finite = std::isfinite(s->h_xx) && std::isfinite(s->h_xy) && std::isfinite(s->h_yy);
    const double det = s->h_xx * s->h_yy - s->h_xy * s->h_xy;
    if (!(finite && s->h_xx > 0.0 && s->h_yy > 0.0 && det > 0.0 && std::isfinite(det)))
      return erpl_fail(ERPL_ERR_INVALID, "spec->h_xx = %g, spec->h_xy = %g, spec->h_yy = %g: not a finite positive definite matrix",
                       s->h_xx, s->h_xy, s->h_yy);
  }
  ERPL_TRY(check_levels(s->level, s->n_levels, ERPL_DENSITY_MAX_LEVELS));
  ERPL_TRY(check_int(s->n_zones, "n_zones", -1, 0, ERPL_DENSITY_MAX_ZONES));
  if (s->n_zones > 0 && s->zone_first[0] != 0)
    return erpl_fail(ERPL_ERR_INVALID, "spec->zone_first[0] = %d: the first zone starts at vertex 0", s->zone_first[0]);
  for (int z = 0; z < s->n_zones; ++z) {
    const int first = s->zone_first[z], end = s->zone_first[z + 1];
    if (end < first)
      return erpl_fail(ERPL_ERR_INVALID, "spec->zone_first[%d] = %d is below spec->zone_first[%d] = %d", z + 1, end, z, first);
    if (end - first < 3)
      return erpl_fail(ERPL_ERR_INVALID, "spec->zone_first[%d] = %d, spec->zone_first[%d] = %d: zone %d has %d vertices, a polygon needs 3",
                       z, first, z + 1, end, z, end - first);
    if (end > ERPL_DENSITY_MAX_VERTICES)
      return erpl_fail(ERPL_ERR_INVALID, "spec->zone_first[%d] = %d: more than %d vertices together", z + 1, end,
                       ERPL_DENSITY_MAX_VERTICES);
    for (int v = first; v < end; ++v)
      if (!(std::isfinite(s->zone_x[v]) && std::isfinite(s->zone_y[v])))
        return erpl_fail(ERPL_ERR_INVALID, "spec->zone_x[%d] = %g, spec->zone_y[%d] = %g: not a finite vertex (zone %d)", v,
                         s->zone_x[v], v, s->zone_y[v], z);
  }
  return ERPL_OK;
}

}  // namespace

extern "C" {

int erpl_mc_impact_density_defaults(erpl_density_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->row_x = ERPL_SUM_IMPACT_X; spec->row_y = ERPL_SUM_IMPACT_Y;
  spec->nodes_x = spec->nodes_y = 128;
  spec->lo_x = spec->hi_x = spec->lo_y = spec->hi_y = NAN;   // from the data
  spec->pad = 3.0;
  spec->bandwidth = ERPL_BW_SCOTT;
  spec->bw_scale = 1.0;
  spec->h_xx = spec->h_yy = 1.0;
  spec->n_levels = 3;
  spec->level[0] = 0.5; spec->level[1] = 0.9; spec->level[2] = 0.99;
  return ERPL_OK;
}

int erpl_mc_impact_density(erpl_ctx* c, const double* summary, const uint8_t* mask, int64_t n, const erpl_density_spec* spec,
                           double* grid_x, double* grid_y, double* density, erpl_density* result, double* sample_density,
                           void* stream) {
  NEED(spec);
  ERPL_TRY(check_density_spec(spec));
  ERPL_TRY(check_n(n, (1ll << 31) - 1, ": the select carries 31-bit sample indices"));
  NEED(summary); NEED(grid_x); NEED(grid_y); NEED(density); NEED(result); NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int nx = spec->nodes_x, ny = spec->nodes_y;
  const size_t nodes = (size_t)nx * (size_t)ny;
  const bool want_samples = spec->n_levels > 0 || sample_density;

  size_t temp_bytes = 0;
  LAUNCH_TRY(erpl_boot_temp_bytes(n, &temp_bytes), "select sizing failed");
  const ErplDensLayout at = erpl_dens_layout(n, (int64_t)nodes, want_samples, sample_density != nullptr, temp_bytes);
  ERPL_TRY(c->dens.first_use());
  if (want_samples) ERPL_TRY(c->ana.first_use());   // the selection's block
  ERPL_TRY(c->dens.grow(at.need));
  char* buf = c->dens.buf;
  DensHost& h = *c->dens.host;
  uint32_t* src = (uint32_t*)(buf + at.src);
  double* pts = (double*)(buf + at.pts);
  double* nodes_uv = (double*)(buf + at.nodes);
  double* dens = (double*)(buf + at.dens);
  double* row = sample_density ? sample_density : (double*)(buf + at.row);
  double* partial = (double*)(buf + at.part);

  ErplDensArgs a;
  memset(&a, 0, sizeof(a));
  a.summary = summary; a.mask = mask; a.work = c->dens.work; a.pop = (uint8_t*)(buf + at.pop); a.n = n;
  a.row_x = spec->row_x; a.row_y = spec->row_y; a.n_zones = spec->n_zones;
  ErplBootPrep p;   // the select of erpl_mc_bootstrap: pop -> src and the count, in sample order
  memset(&p, 0, sizeof(p));
  p.pop = a.pop; p.src = src; p.count = (unsigned long long*)(buf + at.count); p.temp = buf + at.temp;
  p.temp_bytes = at.temp_bytes; p.n = n;
  KERNEL_TRY(erpl_launch_dens_population(a, stream));
  LAUNCH_TRY(erpl_launch_boot_compact(p, stream), "select failed");
  KERNEL_TRY(erpl_launch_dens_moments(a, src, p.count, pts, stream));
  HIP_TRY(hipMemcpyAsync(&h.mom, &c->dens.work->mom, sizeof(ErplDensMoments), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  // what the host settles in double: S, H, whether the estimate is solid, the map, the ranges and the nodes
  const double nan = NAN;
  const int64_t m = (int64_t)h.mom.count;
  memset(result, 0, sizeof(*result));
  const double dof = (double)(m - 1);   // 0 for m == 1: S is NaN there
  const bool any = finish_cloud(result, h.mom.count, h.mom.mean_x, h.mom.mean_y, h.mom.sxx / dof, h.mom.sxy / dof, h.mom.syy / dof);
  double hxx = spec->h_xx, hxy = spec->h_xy, hyy = spec->h_yy;
  if (spec->bandwidth == ERPL_BW_SCOTT) {
    const double factor = spec->bw_scale * pow((double)m, -1.0 / 6.0), f2 = factor * factor;
    hxx = f2 * result->cov_xx; hxy = f2 * result->cov_xy; hyy = f2 * result->cov_yy;
  }
  const double det = hxx * hyy - hxy * hxy;
  const bool solid = any && std::isfinite(hxx) && std::isfinite(hxy) && std::isfinite(hyy) && std::isfinite(det) &&
                     hxx > 0.0 && hyy > 0.0 && det > 1e-12 * hxx * hyy && !(spec->bandwidth == ERPL_BW_SCOTT && m < 3);
  result->solid = solid ? 1 : 0;
  result->h_xx = any ? hxx : nan; result->h_xy = any ? hxy : nan; result->h_yy = any ? hyy : nan;
  result->det = any ? det : nan;
  const double norm = solid ? 1.0 / ((double)m * (2.0 * M_PI) * sqrt(det)) : nan;
  result->norm = norm;
  const bool auto_x = std::isnan(spec->lo_x), auto_y = std::isnan(spec->lo_y);
  const double pad_x = solid ? spec->pad * sqrt(hxx) : 0.0, pad_y = solid ? spec->pad * sqrt(hyy) : 0.0;
  double lo_x = spec->lo_x, hi_x = spec->hi_x, lo_y = spec->lo_y, hi_y = spec->hi_y;
  if (!settle_range(auto_x, h.mom.min_x - pad_x, h.mom.max_x + pad_x, &lo_x, &hi_x))
    return erpl_fail(ERPL_ERR_INVALID, "spec->row_x = %d: the range of the counted values, %g to %g, is wider than a double holds",
                     spec->row_x, lo_x, hi_x);
  if (!settle_range(auto_y, h.mom.min_y - pad_y, h.mom.max_y + pad_y, &lo_y, &hi_y))
    return erpl_fail(ERPL_ERR_INVALID, "spec->row_y = %d: the range of the counted values, %g to %g, is wider than a double holds",
                     spec->row_y, lo_y, hi_y);
  result->lo_x = lo_x; result->hi_x = hi_x; result->lo_y = lo_y; result->hi_y = hi_y;
  memset(&h.in, 0, sizeof(h.in));
  fill_edges(lo_x, hi_x, nx - 1, h.in.grid_x);   // np.linspace(lo, hi, nodes)
  fill_edges(lo_y, hi_y, ny - 1, h.in.grid_y);
  const int n_vert = spec->n_zones > 0 ? spec->zone_first[spec->n_zones] : 0;
  memcpy(h.in.zone_x, spec->zone_x, (size_t)n_vert * sizeof(double));
  memcpy(h.in.zone_y, spec->zone_y, (size_t)n_vert * sizeof(double));
  for (int z = 0; z <= spec->n_zones; ++z) h.in.zone_first[z] = spec->zone_first[z];
  HIP_TRY(hipMemcpyAsync(&c->dens.work->in, &h.in, sizeof(ErplDensIn), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(&c->dens.work->out, 0, sizeof(ErplDensOut), st));
  if (spec->n_zones > 0) KERNEL_TRY(erpl_launch_dens_zones(a, stream));

  if (solid) {
    // H = C C': u = dx / c11, v = (dy - c21 u) / c22
    const double c11 = sqrt(hxx), c21 = hxy / c11, c22 = sqrt(hyy - c21 * c21);
    ErplDensMap map;
    map.mean_x = h.mom.mean_x; map.mean_y = h.mom.mean_y;
    map.w11 = 1.0 / c11; map.w22 = 1.0 / c22; map.w21 = -c21 * map.w11 * map.w22;
    KERNEL_TRY(erpl_launch_dens_whiten(pts, m, map, stream));
    KERNEL_TRY(erpl_launch_dens_nodes(c->dens.work, nx, ny, map, nodes_uv, stream));
    KERNEL_TRY(erpl_launch_dens_pairs(nodes_uv, (int64_t)nodes, pts, m, norm, partial, dens, nullptr, stream));
    KERNEL_TRY(erpl_launch_dens_peak(c->dens.work, dens, (int64_t)nodes, stream));
  }
  double q[ERPL_ANALYSIS_MAX_Q] = {0};   // the density below which 1 - level of the samples lie bounds the region of that content
  for (int k = 0; k < spec->n_levels; ++k) q[k] = 1.0 - spec->level[k];
  if (want_samples) {
    KERNEL_TRY(erpl_launch_dens_fill_nan(row, n, stream));
    if (solid) {
      KERNEL_TRY(erpl_launch_dens_pairs(pts, m, pts, m, norm, partial, row, src, stream));
      // the f_j as a one-row summary through the moment passes and the selection of erpl_mc_analyze
      ERPL_TRY(describe_rows(c, row, a.pop, n, nullptr, 1, q, spec->n_levels, c->ana.host, st));
    }
  }
  HIP_TRY(hipMemcpyAsync(&h.out, &c->dens.work->out, sizeof(ErplDensOut), hipMemcpyDeviceToHost, st));
  if (solid) HIP_TRY(hipMemcpyAsync(density, dens, 8 * nodes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  memcpy(grid_x, h.in.grid_x, (size_t)nx * sizeof(double));
  memcpy(grid_y, h.in.grid_y, (size_t)ny * sizeof(double));
  if (!solid) for (size_t k = 0; k < nodes; ++k) density[k] = nan;
  for (int z = 0; z < ERPL_DENSITY_MAX_ZONES; ++z) result->zone_inside[z] = z < spec->n_zones ? (int64_t)h.out.zone_inside[z] : 0;
  const double cell = ((hi_x - lo_x) / (double)(nx - 1)) * ((hi_y - lo_y) / (double)(ny - 1));
  result->peak = solid ? h.out.peak : nan;
  result->grid_mass = solid ? h.out.sum * cell : nan;
  result->peak_ix = solid ? (int32_t)((int64_t)h.out.peak_at / ny) : -1;
  result->peak_iy = solid ? (int32_t)((int64_t)h.out.peak_at % ny) : -1;
  const bool described = solid && want_samples;
  finish_row_stats(described ? c->ana.host->row[0] : ErplAnaRow(), q, spec->n_levels, described, result->sample_density);
  return ERPL_OK;
}

// The weighted map: the host half of erpl_mc_impact_density above with the passes of erpl_density_w.hip where a weight enters
// (population, moments, zones, pairs, regions) and the launchers of erpl_density.hip where none does (whiten, nodes, fold, peak,
// fill_nan, on the ErplDensWork inside the block).
int erpl_mc_impact_density_weighted(erpl_ctx* c, const double* summary, const uint8_t* mask, const int64_t* weights, int64_t n,
                                    const erpl_density_spec* spec, double* grid_x, double* grid_y, double* density,
                                    erpl_density_w* result, double* sample_density, void* stream) {
  NEED(spec);
  ERPL_TRY(check_density_spec(spec));
  ERPL_TRY(check_n(n, (1ll << 31) - 1, ": the select carries 31-bit sample indices"));
  NEED(summary); NEED(grid_x); NEED(grid_y); NEED(density); NEED(weights); NEED(result); NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int nx = spec->nodes_x, ny = spec->nodes_y;
  const size_t nodes = (size_t)nx * (size_t)ny;
  const bool want_samples = spec->n_levels > 0 || sample_density;

  size_t temp_bytes = 0;
  LAUNCH_TRY(erpl_boot_temp_bytes(n, &temp_bytes), "select sizing failed");
  const ErplDensWLayout at = erpl_densw_layout(n, (int64_t)nodes, want_samples, sample_density != nullptr, temp_bytes);
  ERPL_TRY(c->densw.first_use());
  ERPL_TRY(c->densw.grow(at.need));
  char* buf = c->densw.buf;
  ErplDensWWork* work = c->densw.work;
  DensWHost& h = *c->densw.host;
  uint32_t* src = (uint32_t*)(buf + at.src);
  double* pts = (double*)(buf + at.pts);
  double* ws = (double*)(buf + at.ws);
  double* nodes_uv = (double*)(buf + at.nodes);
  double* dens = (double*)(buf + at.dens);
  double* row = sample_density ? sample_density : (double*)(buf + at.row);
  double* partial = (double*)(buf + at.part);

  ErplDensWArgs a;
  memset(&a, 0, sizeof(a));
  a.summary = summary; a.mask = mask; a.weights = weights; a.work = work; a.pop = (uint8_t*)(buf + at.pop); a.n = n;
  a.row_x = spec->row_x; a.row_y = spec->row_y; a.n_zones = spec->n_zones; a.Q = erpl_rw_q(n);
  ErplBootPrep p;   // the select of erpl_mc_bootstrap: pop -> src and the count, in sample order
  memset(&p, 0, sizeof(p));
  p.pop = a.pop; p.src = src; p.count = (unsigned long long*)(buf + at.count); p.temp = buf + at.temp;
  p.temp_bytes = at.temp_bytes; p.n = n;
  KERNEL_TRY(erpl_launch_densw_population(a, stream));
  LAUNCH_TRY(erpl_launch_boot_compact(p, stream), "select failed");
  KERNEL_TRY(erpl_launch_densw_moments(a, src, p.count, pts, ws, stream));
  HIP_TRY(hipMemcpyAsync(&h.mom, &work->mom, sizeof(ErplDensWMoments), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h.mom.first_bad < (double)n)
    return erpl_fail(ERPL_ERR_INVALID, "weights[%lld] is outside 0 .. 2^%d", (long long)h.mom.first_bad, a.Q);

  // what the host settles in double: the covariance, H, whether the estimate is solid, the map, the ranges and the nodes
  const double nan = NAN;
  const int64_t m = (int64_t)h.mom.count;
  memset(result, 0, sizeof(*result));
  const double s_d = h.mom.s_d, dof = s_d - h.mom.sum_w2 / s_d;   // 0 for one point: the covariance is NaN there
  const bool any = finish_cloud(result, h.mom.count, h.mom.mean_x, h.mom.mean_y, h.mom.sxx / dof, h.mom.sxy / dof, h.mom.syy / dof);
  result->n_masked = (int64_t)h.mom.n_masked; result->n_non_finite = (int64_t)h.mom.n_non_finite;
  result->n_zero = (int64_t)h.mom.n_zero;
  result->sum_w = (int64_t)h.mom.sum_w; result->max_w = (int64_t)h.mom.max_w;
  result->sum_w2 = any ? h.mom.sum_w2 : nan;
  result->ess = any ? s_d * s_d / h.mom.sum_w2 : nan;
  double hxx = spec->h_xx, hxy = spec->h_xy, hyy = spec->h_yy;
  if (spec->bandwidth == ERPL_BW_SCOTT) {
    const double factor = spec->bw_scale * pow(result->ess, -1.0 / 6.0), f2 = factor * factor;
    hxx = f2 * result->cov_xx; hxy = f2 * result->cov_xy; hyy = f2 * result->cov_yy;
  }
  const double det = hxx * hyy - hxy * hxy;
  const bool solid = any && std::isfinite(hxx) && std::isfinite(hxy) && std::isfinite(hyy) && std::isfinite(det) &&
                     hxx > 0.0 && hyy > 0.0 && det > 1e-12 * hxx * hyy && !(spec->bandwidth == ERPL_BW_SCOTT && m < 3);
  result->solid = solid ? 1 : 0;
  result->h_xx = any ? hxx : nan; result->h_xy = any ? hxy : nan; result->h_yy = any ? hyy : nan;
  result->det = any ? det : nan;
  const double norm = solid ? 1.0 / (s_d * (2.0 * M_PI) * sqrt(det)) : nan;
  result->norm = norm;
  const bool auto_x = std::isnan(spec->lo_x), auto_y = std::isnan(spec->lo_y);
  const double pad_x = solid ? spec->pad * sqrt(hxx) : 0.0, pad_y = solid ? spec->pad * sqrt(hyy) : 0.0;
  double lo_x = spec->lo_x, hi_x = spec->hi_x, lo_y = spec->lo_y, hi_y = spec->hi_y;
  if (!settle_range(auto_x, h.mom.min_x - pad_x, h.mom.max_x + pad_x, &lo_x, &hi_x))
    return erpl_fail(ERPL_ERR_INVALID, "spec->row_x = %d: the range of the counted values, %g to %g, is wider than a double holds",
                     spec->row_x, lo_x, hi_x);
  if (!settle_range(auto_y, h.mom.min_y - pad_y, h.mom.max_y + pad_y, &lo_y, &hi_y))
    return erpl_fail(ERPL_ERR_INVALID, "spec->row_y = %d: the range of the counted values, %g to %g, is wider than a double holds",
                     spec->row_y, lo_y, hi_y);
  result->lo_x = lo_x; result->hi_x = hi_x; result->lo_y = lo_y; result->hi_y = hi_y;
  memset(&h.in, 0, sizeof(h.in));
  fill_edges(lo_x, hi_x, nx - 1, h.in.grid_x);   // np.linspace(lo, hi, nodes)
  fill_edges(lo_y, hi_y, ny - 1, h.in.grid_y);
  const int n_vert = spec->n_zones > 0 ? spec->zone_first[spec->n_zones] : 0;
  memcpy(h.in.zone_x, spec->zone_x, (size_t)n_vert * sizeof(double));
  memcpy(h.in.zone_y, spec->zone_y, (size_t)n_vert * sizeof(double));
  for (int z = 0; z <= spec->n_zones; ++z) h.in.zone_first[z] = spec->zone_first[z];
  HIP_TRY(hipMemcpyAsync(&work->d.in, &h.in, sizeof(ErplDensIn), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(&work->d.out, 0, sizeof(ErplDensOut), st));
  HIP_TRY(hipMemsetAsync(&work->out, 0, sizeof(ErplDensWOut), st));
  KERNEL_TRY(erpl_launch_densw_zones(a, pts, ws, m, stream));   // before the points are whitened

  int64_t per_slice = 0;
  if (solid) {
    // H = C C': u = dx / c11, v = (dy - c21 u) / c22
    const double c11 = sqrt(hxx), c21 = hxy / c11, c22 = sqrt(hyy - c21 * c21);
    ErplDensMap map;
    map.mean_x = h.mom.mean_x; map.mean_y = h.mom.mean_y;
    map.w11 = 1.0 / c11; map.w22 = 1.0 / c22; map.w21 = -c21 * map.w11 * map.w22;
    KERNEL_TRY(erpl_launch_dens_whiten(pts, m, map, stream));
    KERNEL_TRY(erpl_launch_dens_nodes(&work->d, nx, ny, map, nodes_uv, stream));
    KERNEL_TRY(erpl_launch_densw_pairs(nodes_uv, (int64_t)nodes, pts, ws, m, partial, stream));
    KERNEL_TRY(erpl_launch_dens_fold(partial, erpl_dens_slices(m, (int64_t)nodes, &per_slice), (int64_t)nodes, norm, dens, nullptr, stream));
    KERNEL_TRY(erpl_launch_dens_peak(&work->d, dens, (int64_t)nodes, stream));
  }
  if (want_samples) {
    KERNEL_TRY(erpl_launch_dens_fill_nan(row, n, stream));
    if (solid) {
      KERNEL_TRY(erpl_launch_densw_pairs(pts, m, pts, ws, m, partial, stream));
      KERNEL_TRY(erpl_launch_dens_fold(partial, erpl_dens_slices(m, m, &per_slice), m, norm, row, src, stream));
      // the region of content level[k] is bounded by the density below which 1 - level[k] of the WEIGHT lies
      unsigned long long rank[ERPL_DENSITY_MAX_LEVELS] = {0};
      for (int k = 0; k < spec->n_levels; ++k) rank[k] = erpl_rw_target(1.0 - spec->level[k], h.mom.sum_w) - 1ull;
      KERNEL_TRY(erpl_launch_densw_regions(a, row, rank, spec->n_levels, stream));
    }
  }
  HIP_TRY(hipMemcpyAsync(&h.peak, &work->d.out, sizeof(ErplDensOut), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&h.out, &work->out, sizeof(ErplDensWOut), hipMemcpyDeviceToHost, st));
  if (solid) HIP_TRY(hipMemcpyAsync(density, dens, 8 * nodes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  memcpy(grid_x, h.in.grid_x, (size_t)nx * sizeof(double));
  memcpy(grid_y, h.in.grid_y, (size_t)ny * sizeof(double));
  if (!solid) for (size_t k = 0; k < nodes; ++k) density[k] = nan;
  for (int z = 0; z < ERPL_DENSITY_MAX_ZONES; ++z) {
    result->zone_w[z] = z < spec->n_zones ? (int64_t)h.out.zone_w[z] : 0;
    result->zone_a2[z] = z < spec->n_zones ? h.out.zone_a2[z] : 0.0;
  }
  const double cell = ((hi_x - lo_x) / (double)(nx - 1)) * ((hi_y - lo_y) / (double)(ny - 1));
  result->peak = solid ? h.peak.peak : nan;
  result->grid_mass = solid ? h.peak.sum * cell : nan;
  result->peak_ix = solid ? (int32_t)((int64_t)h.peak.peak_at / ny) : -1;
  result->peak_iy = solid ? (int32_t)((int64_t)h.peak.peak_at % ny) : -1;
  const bool described = solid && want_samples;
  for (int k = 0; k < ERPL_DENSITY_MAX_LEVELS; ++k) {
    const bool has = described && k < spec->n_levels;
    result->threshold[k] = has ? double_of_key(h.out.key[k]) : nan;
    result->content_w[k] = has ? (int64_t)h.out.content_w[k] : 0;
  }
  result->f_min = described ? h.out.f_min : nan;
  result->f_max = described ? h.out.f_max : nan;
  return ERPL_OK;
}

}  // extern "C"

// ------------------------------------------------- erpl_mc_corridor_resample, erpl_mc_corridor_bands
namespace {

// every field of the spec, for both calls: channels, nodes, flags, t0, dt, quantiles - in that order
int check_corridor_spec(const erpl_corridor_spec* s) {
  ERPL_TRY(check_int(s->n_channels, "n_channels", -1, 1, ERPL_CORRIDOR_MAX_CHANNELS));
  for (int j = 0; j < s->n_channels; ++j) {
    ERPL_TRY(check_int(s->channels[j], "channels", j, 0, ERPL_CH_COUNT - 1));
    for (int k = 0; k < j; ++k)
      if (s->channels[k] == s->channels[j])
        return erpl_fail(ERPL_ERR_INVALID, "spec->channels[%d] = %d is listed twice", j, s->channels[j]);
  }
  ERPL_TRY(check_int(s->n_nodes, "n_nodes", -1, 1, ERPL_CORRIDOR_MAX_NODES));
  if (s->flags & ~ERPL_CORRIDOR_HOLD_END) return erpl_fail(ERPL_ERR_INVALID, "spec->flags = %d: ERPL_CORRIDOR_HOLD_END or 0", s->flags);
  if (!std::isfinite(s->t0)) return erpl_fail(ERPL_ERR_INVALID, "spec->t0 = %g is not finite", s->t0);
  if (!(std::isfinite(s->dt) && s->dt > 0.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->dt = %g: finite and > 0", s->dt);
  return check_quantiles(s->q, s->n_q);
}

}  // namespace

extern "C" {

int erpl_mc_corridor_defaults(erpl_corridor_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->n_channels = 3;
  spec->channels[0] = ERPL_CH_Z; spec->channels[1] = ERPL_CH_DOWNRANGE; spec->channels[2] = ERPL_CH_SPEED;
  spec->n_nodes = 256;
  spec->t0 = 0.0; spec->dt = 1.0;
  spec->n_q = 5;
  const double q[5] = {0.05, 0.25, 0.5, 0.75, 0.95};   // erpl_mc_analysis_defaults
  for (int j = 0; j < 5; ++j) spec->q[j] = q[j];
  return ERPL_OK;
}

int erpl_mc_corridor_resample(erpl_ctx* c, const erpl_out* out, const erpl_corridor_spec* spec, double* values, int64_t ld,
                              int64_t col0, void* stream) {
  NEED(spec);
  ERPL_TRY(check_corridor_spec(spec));
  NEED(out);
  if (out->n_traj < 0 || out->n_traj > 2147483647LL)
    return erpl_fail(ERPL_ERR_INVALID, "n_traj = %lld out of range 0..2^31 - 1", (long long)out->n_traj);
  if (col0 < 0) return erpl_fail(ERPL_ERR_INVALID, "col0 = %lld is negative", (long long)col0);
  if (ld < out->n_traj || col0 > ld - out->n_traj)
    return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below col0 + n_traj = %lld + %lld", (long long)ld, (long long)col0,
                     (long long)out->n_traj);
  NEED(values);
  if (out->n_traj > 0) {
    if (out->traj_cap < 1)
      return erpl_fail(ERPL_ERR_INVALID, "traj_cap = %lld: at least one record per trajectory", (long long)out->traj_cap);
    NEED_AS(out->traj, "traj"); NEED_AS(out->traj_len, "traj_len");
  }
  NEED_AS(c, "ctx");
  if (out->n_traj == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  ErplCorridorResampleArgs a;
  memset(&a, 0, sizeof(a));
  a.traj = out->traj; a.traj_len = out->traj_len; a.values = values;
  a.n_traj = out->n_traj; a.traj_cap = out->traj_cap; a.ld = ld; a.col0 = col0;
  a.n_channels = spec->n_channels; a.n_nodes = spec->n_nodes; a.hold = (spec->flags & ERPL_CORRIDOR_HOLD_END) ? 1 : 0;
  for (int j = 0; j < spec->n_channels; ++j) a.channels[j] = spec->channels[j];
  a.t0 = spec->t0; a.dt = spec->dt;
  KERNEL_TRY(erpl_launch_corridor_resample(a, stream));
  return ERPL_OK;
}

int erpl_mc_corridor_bands(erpl_ctx* c, const double* values, const uint8_t* mask, int64_t m, int64_t ld,
                           const erpl_corridor_spec* spec, erpl_row_stats* bands, int64_t* n_counted, void* stream) {
  NEED(spec);
  ERPL_TRY(check_corridor_spec(spec));
  if (m <= 0 || m > 2147483647LL) return erpl_fail(ERPL_ERR_INVALID, "m = %lld outside 1..2^31 - 1", (long long)m);
  if (ld < m) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below m = %lld", (long long)ld, (long long)m);
  NEED(values); NEED(bands); NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int rows = spec->n_channels * spec->n_nodes;
  // one piece: a row record per (channel, node) and the record of the column count behind them
  const size_t bytes = ((size_t)rows + 1) * sizeof(ErplAnaRow);
  ERPL_TRY(c->corridor.grow(bytes));
  ErplCorridorBandsArgs a;
  memset(&a, 0, sizeof(a));
  a.values = values; a.mask = mask; a.out = (ErplAnaRow*)c->corridor.buf; a.m = m; a.ld = ld; a.rows = rows; a.n_q = spec->n_q;
  for (int k = 0; k < spec->n_q; ++k) a.q[k] = spec->q[k];
  KERNEL_TRY(erpl_launch_corridor_bands(a, stream));
  std::vector<ErplAnaRow> h((size_t)rows + 1);
  HIP_TRY(hipMemcpyAsync(h.data(), a.out, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int r = 0; r < rows; ++r) finish_row_stats(h[(size_t)r], spec->q, spec->n_q, true, bands[r]);
  if (n_counted) *n_counted = (int64_t)h[(size_t)rows].count;
  return ERPL_OK;
}

// ------------------------------------------------- erpl_mc_corridor_depth
int erpl_mc_corridor_depth_defaults(erpl_depth_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->central = 0.5;
  spec->factor = 1.5;
  return ERPL_OK;
}

int erpl_mc_corridor_depth(erpl_ctx* c, const double* values, int64_t ld, const uint8_t* mask, int64_t m, const erpl_depth_spec* spec,
                           erpl_depth_result* result, erpl_depth_row* rows, double* depth, double* mei, int32_t* nodes, int32_t* n_out,
                           int32_t* first_out, uint8_t* central, void* stream) {
  NEED(spec); NEED(values); NEED(result); NEED(rows); NEED(depth); NEED(mei); NEED(nodes); NEED(n_out); NEED(first_out); NEED(central);
  if (m <= 0 || m > 2147483647LL) return erpl_fail(ERPL_ERR_INVALID, "m = %lld outside 1..2^31 - 1", (long long)m);
  if (ld < m) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below m = %lld", (long long)ld, (long long)m);
  ERPL_TRY(check_int(spec->n_channels, "n_channels", -1, 1, ERPL_DEPTH_MAX_CHANNELS));
  ERPL_TRY(check_int(spec->n_nodes, "n_nodes", -1, 1, ERPL_DEPTH_MAX_NODES));
  if (!(spec->central > 0.0 && spec->central <= 1.0)) return erpl_fail(ERPL_ERR_INVALID, "spec->central = %g outside (0, 1]", spec->central);
  if (!(spec->factor >= 0.0 && std::isfinite(spec->factor)))
    return erpl_fail(ERPL_ERR_INVALID, "spec->factor = %g: finite and >= 0", spec->factor);
  if (spec->lds_limit < 0) return erpl_fail(ERPL_ERR_INVALID, "spec->lds_limit = %d is negative", spec->lds_limit);
  NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int C = spec->n_channels, T = spec->n_nodes;

  const ErplDepthLayout sizing = erpl_depth_layout(m, C, T, spec->lds_limit, 0);
  size_t temp_bytes = 0;
  LAUNCH_TRY(erpl_depth_temp_bytes(m, sizing.group, &temp_bytes), "sizing the sorts failed");
  const ErplDepthLayout at = erpl_depth_layout(m, C, T, spec->lds_limit, temp_bytes);
  ERPL_TRY(c->depth.grow(at.need));
  char* buf = c->depth.buf;
  ErplDepthArgs a;
  memset(&a, 0, sizeof(a));
  a.values = values; a.mask = mask; a.m = m; a.ld = ld; a.n_channels = C; a.n_nodes = T;
  a.central = spec->central; a.factor = spec->factor;
  a.depth = depth; a.mei = mei; a.nodes = nodes; a.n_out = n_out; a.first_out = first_out; a.central_flag = central;
  a.pair = (uint32_t*)(buf + at.pair); a.rown = (int32_t*)(buf + at.rown); a.keys = (unsigned long long*)(buf + at.keys);
  a.offs = (uint32_t*)(buf + at.offs); a.temp = buf + at.temp; a.temp_bytes = temp_bytes;
  a.chan = (ErplDepthChan*)(buf + at.chan); a.rows = (erpl_depth_row*)(buf + at.rows);
  a.count = (unsigned long long*)(buf + at.count);
  a.group = at.group; a.lds = at.lds ? 1 : 0;
  KERNEL_TRY(erpl_launch_depth(a, stream));
  ErplDepthChan chan[ERPL_DEPTH_MAX_CHANNELS];
  unsigned long long masked = 0ull;
  HIP_TRY(hipMemcpyAsync(chan, a.chan, (size_t)C * sizeof(ErplDepthChan), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(rows, a.rows, (size_t)C * T * sizeof(erpl_depth_row), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&masked, a.count, sizeof(masked), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memset(result, 0, sizeof(*result));
  result->m = m;
  result->n_masked = (int64_t)masked;
  for (int k = 0; k < ERPL_DEPTH_MAX_CHANNELS; ++k) {
    const bool in = k < C;
    result->n_defined[k] = in ? chan[k].n_defined : 0;
    result->n_central[k] = in ? chan[k].n_central : 0;
    result->n_outliers[k] = in ? (int64_t)chan[k].n_outliers : 0;
    result->median[k] = in ? chan[k].median : -1;
    result->threshold[k] = in ? chan[k].threshold : (double)NAN;
    result->depth_max[k] = in ? chan[k].depth_max : (double)NAN;
  }
  return ERPL_OK;
}

}  // extern "C"

// ------------------------------------------------- erpl_mc_sobol
extern "C" {

int erpl_mc_sobol_defaults(erpl_sobol_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->n_rows = 3;   // outputs every flight has, tumbling or not
  spec->rows[0] = ERPL_SUM_FIRST_APOGEE_ALT; spec->rows[1] = ERPL_SUM_FIRST_APOGEE_TIME; spec->rows[2] = ERPL_SUM_RAIL_EXIT_SPEED;
  spec->replicates = 1000;
  spec->level = 0.95;
  spec->seed = 0;
  return ERPL_OK;
}

int erpl_mc_sobol(erpl_ctx* c, const double* summary, const double* extra, const uint8_t* mask, int64_t n_base, int64_t ld,
                  const erpl_sobol_spec* spec, erpl_sobol* result, double* replicates_out, void* stream) {
  NEED(spec); NEED(summary); NEED(result);
  if (n_base <= 0) return erpl_fail(ERPL_ERR_INVALID, "n_base = %lld: need at least one design row", (long long)n_base);
  ERPL_TRY(check_int(spec->n_factors, "n_factors", -1, 1, ERPL_SOBOL_MAX_FACTORS));
  const int k = spec->n_factors;
  if (n_base >= ((1ll << 31) + k + 1) / (k + 2))   // (k + 2) n_base >= 2^31, without the product
    return erpl_fail(ERPL_ERR_INVALID, "(spec->n_factors + 2) * n_base = %d * %lld is 2^31 or more: the records carry 31-bit indices",
                     k + 2, (long long)n_base);
  const int64_t flights = (int64_t)(k + 2) * n_base;
  if (ld < flights)
    return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below (spec->n_factors + 2) * n_base = %lld", (long long)ld, (long long)flights);
  ERPL_TRY(check_row_list(spec->rows, spec->n_rows, 1, ERPL_SOBOL_MAX_ROWS, ERPL_SOBOL_ROW_EXTRA));
  for (int j = 0; j < spec->n_rows; ++j)
    if (spec->rows[j] == ERPL_SOBOL_ROW_EXTRA && !extra)
      return erpl_fail(ERPL_ERR_INVALID, "extra is NULL but spec->rows[%d] = %d (ERPL_SOBOL_ROW_EXTRA)", j, spec->rows[j]);
  ERPL_TRY(check_int(spec->replicates, "replicates", -1, 0, ERPL_SOBOL_MAX_REPLICATES));
  if (replicates_out && spec->replicates == 0) return erpl_fail(ERPL_ERR_INVALID, "replicates_out is given but spec->replicates = 0");
  if (spec->replicates > 0 && !(spec->level > 0.0 && spec->level < 1.0))
    return erpl_fail(ERPL_ERR_INVALID, "spec->level = %g outside (0, 1)", spec->level);
  NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int R = spec->n_rows, ns = 2 + 2 * k, n_stats = R * ns, B = spec->replicates;
  const size_t un = (size_t)n_base, uB = (size_t)B;

  size_t temp_bytes = 0;
  LAUNCH_TRY(erpl_boot_select_bytes(n_base, &temp_bytes), "select sizing failed");
  const ErplSobolLayout at = erpl_sobol_layout(n_base, k, R, B, replicates_out != nullptr, temp_bytes);
  ERPL_TRY(c->corr.first_use());   // the population pass and its counters
  ERPL_TRY(c->sobol.first_use());
  ERPL_TRY(c->sobol.grow(at.need));
  char* buf = c->sobol.buf;
  SobolHost& h = *c->sobol.host;

  ErplSobolArgs a;
  memset(&a, 0, sizeof(a));
  a.work = c->sobol.work; a.rep = replicates_out ? replicates_out : (double*)(buf + at.rep);
  a.seed = spec->seed; a.n_base = n_base; a.n_rows = R; a.k = k; a.replicates = B;
  // per row: the population bytes, its counters and the extremes of the blocks A and B, then the select
  for (int j = 0; j < R; ++j) {
    a.var[j] = spec->rows[j] == ERPL_SOBOL_ROW_EXTRA ? extra : summary + (size_t)spec->rows[j] * (size_t)ld;
    a.src[j] = (uint32_t*)(buf + at.src[j]);
    a.rec[j] = (double*)(buf + at.rec[j]);
    ErplCorrArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.mask = mask; pa.n = n_base; pa.n_vars = k + 2; pa.work = c->corr.work; pa.pop = (uint8_t*)(buf + at.pop) + (size_t)j * un;
    for (int b = 0; b < k + 2; ++b) pa.var[b] = a.var[j] + (size_t)b * un;
    KERNEL_TRY(erpl_launch_corr_population(pa, stream));
    HIP_TRY(hipMemcpyAsync(h.counter[j], &c->corr.work->out.counter[0], sizeof(h.counter[j]), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h.vmin[j], &c->corr.work->out.vmin[0], sizeof(h.vmin[j]), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h.vmax[j], &c->corr.work->out.vmax[0], sizeof(h.vmax[j]), hipMemcpyDeviceToHost, st));
    ErplBootPrep p;
    memset(&p, 0, sizeof(p));
    p.pop = pa.pop; p.src = (uint32_t*)(buf + at.src[j]); p.count = (unsigned long long*)(buf + at.count) + j;
    p.temp = buf + at.temp; p.temp_bytes = at.temp_bytes; p.n = n_base;
    LAUNCH_TRY(erpl_launch_boot_compact(p, stream), "select failed");
  }
  HIP_TRY(hipStreamSynchronize(st));

  const double nan = NAN;
  memset(result, 0, sizeof(*result));
  result->n_base = n_base; result->n_factors = k; result->n_rows = R; result->replicates = B; result->n_stats = n_stats;
  for (int j = 0; j < ERPL_SOBOL_MAX_ROWS; ++j) {
    erpl_sobol_row& o = result->row[j];
    erpl_boot_stat* stats = &o.mean;   // mean, variance, first[], total[]: one run of erpl_boot_stat
    for (int s = 0; s < 2 + 2 * ERPL_SOBOL_MAX_FACTORS; ++s) {
      stats[s].estimate = stats[s].rep_mean = stats[s].se = stats[s].lo = stats[s].hi = nan;
      stats[s].finite = 0;
    }
    if (j >= R) continue;
    o.count = (int64_t)h.counter[j][0]; o.n_masked = (int64_t)h.counter[j][1]; o.n_non_finite = (int64_t)h.counter[j][2];
    a.m[j] = (uint32_t)h.counter[j][0];
  }

  KERNEL_TRY(erpl_launch_sobol_records(a, stream));
  KERNEL_TRY(erpl_launch_sobol_estimates(a, stream));
  HIP_TRY(hipMemcpyAsync(&h.out, &c->sobol.work->out, sizeof(ErplSobolOut), hipMemcpyDeviceToHost, st));
  if (B > 0) {
    KERNEL_TRY(erpl_launch_sobol_replicates(a, stream));
    // the summary over the replicates: the [n_stats][B] matrix as rows of length B through the one-launch row kernel
    const double tail = (1.0 - spec->level) / 2;
    ErplCorridorBandsArgs g;
    memset(&g, 0, sizeof(g));
    g.values = a.rep; g.out = c->sobol.work->bands; g.m = B; g.ld = B; g.rows = n_stats; g.n_q = 2;
    g.q[0] = tail; g.q[1] = 1.0 - tail;
    KERNEL_TRY(erpl_launch_corridor_bands(g, stream));
    HIP_TRY(hipMemcpyAsync(h.bands, c->sobol.work->bands, (size_t)n_stats * sizeof(ErplAnaRow), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));

  const double tail = (1.0 - spec->level) / 2, interval[2] = {tail, 1.0 - tail};
  for (int j = 0; j < R; ++j) {
    erpl_sobol_row& o = result->row[j];
    erpl_boot_stat* stats = &o.mean;
    const bool any = o.count > 0;
    const double dm = (double)o.count, dm2 = 2.0 * dm;
    const double lo = fmin(h.vmin[j][0], h.vmin[j][1]), hi = fmax(h.vmax[j][0], h.vmax[j][1]);
    o.constant = any && lo == hi ? 1 : 0;
    if (any) {
      const double* sum = h.out.sum[j];
      const double V = o.constant ? 0.0 : sum[1] / dm2;
      const bool flat = o.constant || V == 0.0;
      stats[0].estimate = h.out.f0[j];
      stats[1].estimate = V;
      for (int i = 0; i < k; ++i) {
        stats[2 + i].estimate = flat ? nan : (sum[2 + i] / dm) / V;
        stats[2 + ERPL_SOBOL_MAX_FACTORS + i].estimate = flat ? nan : (sum[2 + k + i] / dm2) / V;
      }
    }
    if (B == 0) continue;
    for (int s = 0; s < ns; ++s) {   // statistic s of the matrix -> its place in the row (total[] starts behind first[32])
      erpl_boot_stat& t = stats[s < 2 + k ? s : s - k + ERPL_SOBOL_MAX_FACTORS];
      const ErplAnaRow& row = h.bands[j * ns + s];
      erpl_row_stats over;
      finish_row_stats(row, interval, 2, true, over);
      t.finite = over.count;
      // the constant rule of erpl_mc_bootstrap: a statistic with min == max over its replicates has no spread
      const bool same = over.count > 0 && row.vmin == row.vmax;
      t.rep_mean = same ? row.vmin : over.mean;
      t.se = over.count == 0 ? nan : (same ? 0.0 : sqrt(row.m2 / (double)(over.count - 1)));
      t.lo = over.quantile[0];
      t.hi = over.quantile[1];
    }
  }
  return ERPL_OK;
}

}  // extern "C"

// ------------------------------------------------- erpl_mc_dependence
namespace {

// What the host makes of the P null values of one measure: the mean in ascending p, the quantile `level` with np.quantile's
// linear interpolation (its _lerp: a + (b - a) t, from t = 1/2 on b - (b - a) (1 - t)), and the values >= estimate.
void finish_null(const double* v, int P, double level, std::vector<double>& sorted, erpl_dep_measure& o) {
  double sum = 0.0;
  int64_t exceed = 0;
  for (int p = 0; p < P; ++p) {
    sum += v[p];
    exceed += v[p] >= o.estimate ? 1 : 0;
  }
  sorted.assign(v, v + P);
  std::sort(sorted.begin(), sorted.end());
  const double pos = (double)(P - 1) * level, below = floor(pos), t = pos - below;
  const int lo = (int)below, hi = lo + 1 < P ? lo + 1 : P - 1;
  const double a = sorted[lo], b = sorted[hi], diff = b - a;
  o.null_mean = sum / (double)P;
  o.null_hi = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
  o.exceed = exceed;
}

}  // namespace

extern "C" {

int erpl_mc_dependence_defaults(erpl_dep_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->n_rows = 3;
  spec->rows[0] = ERPL_SUM_APOGEE_ALT; spec->rows[1] = ERPL_SUM_RANGE; spec->rows[2] = ERPL_SUM_FLIGHT_TIME;
  spec->classes = spec->cells = 16;
  spec->shifts = 200;
  spec->level = 0.95;
  spec->seed = 0;
  return ERPL_OK;
}

int erpl_mc_dependence(erpl_ctx* c, const double* factors, const double* summary, const double* extra, const uint8_t* mask,
                       int64_t n, const erpl_dep_spec* spec, erpl_dependence* result, int64_t* tables, double* class_stats,
                       double* null_out, void* stream) {
  NEED(spec); NEED(factors); NEED(summary); NEED(result);
  ERPL_TRY(check_n(n, (1ll << 31) - 1, ": the sort and the tables carry 31-bit sample indices"));
  ERPL_TRY(check_int(spec->n_factors, "n_factors", -1, 1, ERPL_DEP_MAX_FACTORS));
  ERPL_TRY(check_row_list(spec->rows, spec->n_rows, 1, ERPL_DEP_MAX_ROWS, ERPL_DEP_ROW_EXTRA));
  for (int j = 0; j < spec->n_rows; ++j)
    if (spec->rows[j] == ERPL_DEP_ROW_EXTRA && !extra)
      return erpl_fail(ERPL_ERR_INVALID, "extra is NULL but spec->rows[%d] = %d (ERPL_DEP_ROW_EXTRA)", j, spec->rows[j]);
  ERPL_TRY(check_int(spec->classes, "classes", -1, 2, ERPL_DEP_MAX_CLASSES));
  ERPL_TRY(check_int(spec->cells, "cells", -1, 2, ERPL_DEP_MAX_CELLS));
  ERPL_TRY(check_int(spec->shifts, "shifts", -1, 0, ERPL_DEP_MAX_SHIFTS));
  if (null_out && spec->shifts == 0) return erpl_fail(ERPL_ERR_INVALID, "null_out is given but spec->shifts = 0");
  if (spec->shifts > 0 && !(spec->level > 0.0 && spec->level < 1.0))
    return erpl_fail(ERPL_ERR_INVALID, "spec->level = %g outside (0, 1)", spec->level);
  NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int F = spec->n_factors, R = spec->n_rows, M = spec->classes, H = spec->cells, P = spec->shifts;
  const size_t un = (size_t)n, pairs = (size_t)F * R, n_cstat = pairs * M * 6, n_tab = pairs * M * H, n_null = pairs * 4 * (size_t)P;

  size_t temp_bytes = 0;
  LAUNCH_TRY(erpl_boot_temp_bytes(n, &temp_bytes), "select / radix sort sizing failed");
  const ErplDepLayout at = erpl_dep_layout(n, F, R, M, H, P, temp_bytes);
  ERPL_TRY(c->corr.first_use());   // the population pass and its counters
  ERPL_TRY(c->ana.first_use());    // the moments of the rows
  ERPL_TRY(c->dep.first_use());
  ERPL_TRY(c->dep.grow(at.need));
  char* buf = c->dep.buf;
  DepHost& h = *c->dep.host;

  ErplDepArgs a;
  memset(&a, 0, sizeof(a));
  ErplCorrArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.mask = mask; pa.n = n; pa.n_vars = F + R; pa.work = c->corr.work; pa.pop = (uint8_t*)(buf + at.pop);
  for (int f = 0; f < F; ++f) a.var[f] = factors + (size_t)f * un;
  for (int j = 0; j < R; ++j) {
    a.var[F + j] = spec->rows[j] == ERPL_DEP_ROW_EXTRA ? extra : summary + (size_t)spec->rows[j] * un;
    a.yd[j] = (double*)(buf + at.yd[j]);
  }
  for (int v = 0; v < F + R; ++v) pa.var[v] = a.var[v];
  KERNEL_TRY(erpl_launch_corr_population(pa, stream));
  HIP_TRY(hipMemcpyAsync(h.counter, &c->corr.work->out.counter[0], sizeof(h.counter), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t m = (int64_t)h.counter[0];

  const double nan = NAN;
  memset(result, 0, sizeof(*result));
  result->n = n; result->count = m; result->n_masked = (int64_t)h.counter[1]; result->n_non_finite = (int64_t)h.counter[2];
  result->n_factors = F; result->n_rows = R; result->classes = M; result->cells = H; result->shifts = P;
  for (int j = 0; j < ERPL_DEP_MAX_ROWS; ++j) {
    result->row_mean[j] = result->row_ss[j] = nan;
    for (int f = 0; f < ERPL_DEP_MAX_FACTORS; ++f) {
      erpl_dep_pair& o = result->pair[j][f];
      for (erpl_dep_measure* q : {&o.delta, &o.ks_max, &o.ks_median, &o.mi}) q->estimate = q->null_mean = q->null_hi = nan;
      o.eta2 = o.eta2_adj = o.f_stat = nan;
    }
  }
  const bool nulls = P > 0 && m >= 2;
  if (null_out && !nulls) std::fill(null_out, null_out + n_null, nan);
  if (m == 0) {   // nothing counted: empty tables, empty classes
    if (tables) std::fill(tables, tables + n_tab, (int64_t)0);
    if (class_stats)
      for (size_t k = 0; k < n_cstat; ++k) class_stats[k] = k % 6 == 0 ? 0.0 : nan;
    return ERPL_OK;
  }

  // mean and sum((y - mean)^2) of every row, by the passes of erpl_mc_analyze with the population bytes as the mask: the
  // summary rows in one launch, `extra` as a one-row summary in a second
  int32_t est_rows[ERPL_DEP_MAX_ROWS];
  int est_of[ERPL_DEP_MAX_ROWS], n_est = 0, has_extra = 0;   // row j of the spec: rows[0].row[est_of[j]], or rows[1].row[0] (-1)
  for (int j = 0; j < R; ++j) {
    if (spec->rows[j] == ERPL_DEP_ROW_EXTRA) { est_of[j] = -1; has_extra = 1; }
    else { est_of[j] = n_est; est_rows[n_est++] = spec->rows[j]; }
  }
  if (n_est > 0) ERPL_TRY(describe_rows(c, summary, pa.pop, n, est_rows, n_est, nullptr, 0, &h.rows[0], st));
  if (has_extra) ERPL_TRY(describe_rows(c, extra, pa.pop, n, nullptr, 1, nullptr, 0, &h.rows[1], st));

  ErplBootPrep p;
  memset(&p, 0, sizeof(p));
  p.pop = pa.pop; p.src = (uint32_t*)(buf + at.src); p.count = (unsigned long long*)(buf + at.count);
  p.temp = buf + at.temp; p.temp_bytes = at.temp_bytes; p.n = n;
  LAUNCH_TRY(erpl_launch_boot_compact(p, stream), "select failed");
  a.src = p.src; a.xc = (uint8_t*)(buf + at.xc); a.yext = (uint8_t*)(buf + at.yext);
  a.keys = (unsigned long long*)(buf + at.keys); a.idx = (uint32_t*)(buf + at.idx);
  a.temp = buf + at.temp; a.temp_bytes = at.temp_bytes;
  a.cstat = (double*)(buf + at.cstat); a.tab = (long long*)(buf + at.tab); a.null = (double*)(buf + at.null);
  a.work = c->dep.work; a.seed = spec->seed; a.x_stride = at.x_stride; a.y_stride = at.y_stride;
  a.m = (uint32_t)m; a.n_factors = F; a.n_rows = R; a.classes = M; a.cells = H; a.shifts = P;
  LAUNCH_TRY(erpl_launch_dep_classes(a, stream), "class pass failed");
  KERNEL_TRY(erpl_launch_dep_tables(a, stream));

  std::vector<double> cstat(n_cstat), own_null;
  HIP_TRY(hipMemcpyAsync(h.est, c->dep.work->est, pairs * sizeof(ErplDepEst), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(cstat.data(), a.cstat, n_cstat * sizeof(double), hipMemcpyDeviceToHost, st));
  if (tables) HIP_TRY(hipMemcpyAsync(tables, a.tab, n_tab * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  const double* null_values = null_out;
  if (nulls) {
    if (!null_out) { own_null.resize(n_null); null_values = own_null.data(); }
    HIP_TRY(hipMemcpyAsync(const_cast<double*>(null_values), a.null, n_null * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));

  std::vector<double> sorted;
  const double dm = (double)m;
  for (int j = 0; j < R; ++j) {
    const ErplAnaRow& row = est_of[j] < 0 ? h.rows[1].row[0] : h.rows[0].row[est_of[j]];
    const bool constant = row.vmin == row.vmax;
    result->row_mean[j] = row.mean;
    result->row_ss[j] = row.m2;
    for (int f = 0; f < F; ++f) {
      const size_t pr = (size_t)j * F + f;
      const ErplDepEst& e = h.est[pr];
      erpl_dep_pair& o = result->pair[j][f];
      o.classes_used = e.classes_used; o.cells_used = e.cells_used; o.delta_num = e.delta_num;
      erpl_dep_measure* ms[4] = {&o.delta, &o.ks_max, &o.ks_median, &o.mi};
      for (int k = 0; k < 4; ++k) {
        ms[k]->estimate = e.v[k];
        if (nulls) finish_null(null_values + (pr * 4 + k) * (size_t)P, P, spec->level, sorted, *ms[k]);
      }
      // the variance share: B over the classes in ascending order
      double* cs = cstat.data() + pr * M * 6;
      double between = 0.0;
      for (int cl = 0; cl < M; ++cl) {
        if (cs[cl * 6] > 0.0) {
          const double dev = cs[cl * 6 + 1] - row.mean;
          between += cs[cl * 6] * (dev * dev);
          cs[cl * 6 + 2] = sqrt(cs[cl * 6 + 2] / cs[cl * 6]);   // the population std of the class
        }
      }
      const int k = e.classes_used;
      if (!constant) {
        if (k < 2) {
          o.eta2 = 0.0;
        } else {
          o.eta2 = between / row.m2;
          if (m > k) {
            const double dfw = (double)(m - k);
            o.eta2_adj = 1.0 - ((1.0 - o.eta2) * (dm - 1.0)) / dfw;
            o.f_stat = (between / (double)(k - 1)) / ((row.m2 - between) / dfw);
          }
        }
      }
    }
  }
  if (class_stats) memcpy(class_stats, cstat.data(), n_cstat * sizeof(double));
  return ERPL_OK;
}

}  // extern "C"

// ------------------------------------------------- erpl_mc_compare
namespace {

typedef unsigned __int128 u128;

// mean (ascending p) and the order statistic `level` (finish_null's interpolation) of the P null values of one test
void cmp_null(const std::vector<double>& v, double level, std::vector<double>& sorted, erpl_cmp_test& o) {
  const int P = (int)v.size();
  double sum = 0.0;
  for (int p = 0; p < P; ++p) sum += v[p];
  sorted = v;
  std::sort(sorted.begin(), sorted.end());
  const double pos = (double)(P - 1) * level, below = floor(pos), t = pos - below;
  const int lo = (int)below, hi = lo + 1 < P ? lo + 1 : P - 1;
  const double a = sorted[lo], b = sorted[hi], diff = b - a;
  o.null_mean = sum / (double)P;
  o.null_hi = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
  o.p_value = (double)(o.exceed + 1) / (double)(P + 1);
}

// T of Cramer-von Mises from the exact sums of (2 r - 2 c)^2: G = 3 (m_a S_A + m_b S_B) - 2 m_a m_b (4 m_a m_b - 1) over
// 12 m_a m_b N, in integers while they fit (N <= 2^30: G < 2^124)
double cmp_cvm(const ErplCmpRank& r, int64_t m_a, int64_t m_b) {
  const int64_t N = m_a + m_b;
  const u128 sa = ((u128)r.sa_hi << 64) | r.sa_lo, sb = ((u128)r.sb_hi << 64) | r.sb_lo;
  if (N <= (1ll << 30)) {
    const u128 mm = (u128)m_a * (u128)m_b;
    const __int128 g = (__int128)(3 * ((u128)m_a * sa + (u128)m_b * sb)) - (__int128)(2 * mm * (4 * mm - 1));
    return (double)g / (double)(12 * mm * (u128)N);
  }
  const long double la = (long double)m_a, lb = (long double)m_b, ln = (long double)N;
  const long double u = (la * (long double)sa + lb * (long double)sb) / 4.0L;
  return (double)(u / (la * lb * ln) - (4.0L * la * lb - 1.0L) / (6.0L * ln));
}

}  // namespace

extern "C" {

int erpl_mc_compare_defaults(erpl_cmp_spec* spec) {
  NEED(spec);
  memset(spec, 0, sizeof(*spec));
  spec->n_rows = 3;
  spec->rows[0] = ERPL_SUM_APOGEE_ALT; spec->rows[1] = ERPL_SUM_RANGE; spec->rows[2] = ERPL_SUM_FLIGHT_TIME;
  spec->n_q = 5;
  const double q[5] = {0.05, 0.25, 0.5, 0.75, 0.95};   // erpl_mc_analysis_defaults
  for (int j = 0; j < 5; ++j) spec->q[j] = q[j];
  spec->row_x = ERPL_SUM_IMPACT_X; spec->row_y = ERPL_SUM_IMPACT_Y;
  spec->permutations = 999;
  spec->level = 0.95;
  spec->seed = 0;
  return ERPL_OK;
}

int erpl_mc_compare_labels(uint64_t seed, int64_t permutation, int64_t m_a, int64_t m_b, uint8_t* out) {
  NEED(out);
  if (m_a < 0) return erpl_fail(ERPL_ERR_INVALID, "m_a = %lld is negative", (long long)m_a);
  if (m_b < 0) return erpl_fail(ERPL_ERR_INVALID, "m_b = %lld is negative", (long long)m_b);
  if (m_a >= (1ll << 32) || m_b >= (1ll << 32) || m_a + m_b == 0 || m_a + m_b >= (1ll << 32))
    return erpl_fail(ERPL_ERR_INVALID, "m_a + m_b = %lld outside 1..2^32 - 1", (long long)(m_a + m_b));
  if (permutation < 0 || permutation > 0xffffffffll)
    return erpl_fail(ERPL_ERR_INVALID, "permutation = %lld outside 0..2^32 - 1", (long long)permutation);
  const uint64_t N = (uint64_t)(m_a + m_b);
  if (m_a == 0 || m_b == 0) {
    memset(out, m_a > 0 ? 1 : 0, N);
    return ERPL_OK;
  }
  std::vector<std::pair<uint64_t, uint64_t>> key(N);
  for (uint64_t i = 0; i < N; ++i) key[i] = {erpl_boot_draw(seed, (uint32_t)permutation, i), i};
  std::vector<std::pair<uint64_t, uint64_t>> pick(key);
  std::nth_element(pick.begin(), pick.begin() + (m_a - 1), pick.end());
  const std::pair<uint64_t, uint64_t> thr = pick[m_a - 1];   // the m_a-th smallest (key, i) pair
  for (uint64_t i = 0; i < N; ++i) out[i] = erpl_cmp_label(key[i].first, i, thr.first, thr.second) ? 1 : 0;
  return ERPL_OK;
}

int erpl_mc_compare(erpl_ctx* c, const double* summary_a, const uint8_t* mask_a, int64_t n_a, const double* summary_b,
                    const uint8_t* mask_b, int64_t n_b, const double* extra_a, const double* extra_b, const erpl_cmp_spec* spec,
                    erpl_compare* result, double* null_out, void* stream) {
  NEED(spec); NEED(summary_a); NEED(summary_b); NEED(result);
  if (n_a <= 0 || n_a >= (1ll << 31))
    return erpl_fail(ERPL_ERR_INVALID, "n_a = %lld outside 1..2^31 - 1: the sort carries 32-bit pooled indices", (long long)n_a);
  if (n_b <= 0 || n_b >= (1ll << 31))
    return erpl_fail(ERPL_ERR_INVALID, "n_b = %lld outside 1..2^31 - 1: the sort carries 32-bit pooled indices", (long long)n_b);
  ERPL_TRY(check_row_list(spec->rows, spec->n_rows, 1, ERPL_CMP_MAX_ROWS, ERPL_CMP_ROW_EXTRA));
  for (int j = 0; j < spec->n_rows; ++j)
    if (spec->rows[j] == ERPL_CMP_ROW_EXTRA && !(extra_a && extra_b))
      return erpl_fail(ERPL_ERR_INVALID, "%s is NULL but spec->rows[%d] = %d (ERPL_CMP_ROW_EXTRA)", extra_a ? "extra_b" : "extra_a", j,
                       spec->rows[j]);
  ERPL_TRY(check_quantiles(spec->q, spec->n_q));
  const bool biv = spec->row_x >= 0;
  if (biv) ERPL_TRY(check_row_pair(spec->row_x, spec->row_y));
  ERPL_TRY(check_int(spec->permutations, "permutations", -1, 0, ERPL_CMP_MAX_PERMUTATIONS));
  if (null_out && spec->permutations == 0) return erpl_fail(ERPL_ERR_INVALID, "null_out is given but spec->permutations = 0");
  if (spec->permutations > 0 && !(spec->level > 0.0 && spec->level < 1.0))
    return erpl_fail(ERPL_ERR_INVALID, "spec->level = %g outside (0, 1)", spec->level);
  NEED_AS(c, "ctx");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int R = spec->n_rows, nq = spec->n_q, P = spec->permutations, V = R + (biv ? 2 : 0);
  const int64_t n_of[2] = {n_a, n_b};
  const double* summary_of[2] = {summary_a, summary_b};
  const double* extra_of[2] = {extra_a, extra_b};
  const uint8_t* mask_of[2] = {mask_a, mask_b};
  const size_t n_null = (size_t)(3 * R + 1) * (size_t)P;

  size_t select_bytes = 0;
  LAUNCH_TRY(erpl_boot_select_bytes(std::max(n_a, n_b), &select_bytes), "select sizing failed");
  const ErplCompareLayout pl = erpl_compare_layout(n_a, n_b, 0, R, P, biv, select_bytes, 0);
  ERPL_TRY(c->corr.first_use());   // the population passes and their counters
  ERPL_TRY(c->ana.first_use());    // the moments and order statistics of the rows
  ERPL_TRY(c->cmp.first_use());
  ERPL_TRY(c->cmp_pop.grow(pl.pop_need));
  char* pbuf = c->cmp_pop.buf;
  CmpHost& h = *c->cmp.host;

  ErplCmpArgs a;
  memset(&a, 0, sizeof(a));
  uint8_t* pop_of[2] = {(uint8_t*)(pbuf + pl.pop_a), (uint8_t*)(pbuf + pl.pop_b)};
  uint32_t* src_of[2] = {(uint32_t*)(pbuf + pl.src_a), (uint32_t*)(pbuf + pl.src_b)};
  for (int s = 0; s < 2; ++s) {
    const size_t un = (size_t)n_of[s];
    const double** var = s == 0 ? a.var_a : a.var_b;
    for (int j = 0; j < R; ++j) var[j] = spec->rows[j] == ERPL_CMP_ROW_EXTRA ? extra_of[s] : summary_of[s] + (size_t)spec->rows[j] * un;
    if (biv) { var[R] = summary_of[s] + (size_t)spec->row_x * un; var[R + 1] = summary_of[s] + (size_t)spec->row_y * un; }
    ErplCorrArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.mask = mask_of[s]; pa.n = n_of[s]; pa.n_vars = V; pa.work = c->corr.work; pa.pop = pop_of[s];
    for (int v = 0; v < V; ++v) pa.var[v] = var[v];
    KERNEL_TRY(erpl_launch_corr_population(pa, stream));
    HIP_TRY(hipMemcpyAsync(h.counter[s], &c->corr.work->out.counter[0], sizeof(h.counter[s]), hipMemcpyDeviceToHost, st));
    ErplBootPrep p;
    memset(&p, 0, sizeof(p));
    p.pop = pop_of[s]; p.src = src_of[s]; p.count = (unsigned long long*)(pbuf + pl.count) + s;
    p.temp = pbuf + pl.sel_temp; p.temp_bytes = pl.sel_bytes; p.n = n_of[s];
    LAUNCH_TRY(erpl_launch_boot_compact(p, stream), "select failed");
  }
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t m_a = (int64_t)h.counter[0][0], m_b = (int64_t)h.counter[1][0], N = m_a + m_b;
  const bool both = m_a > 0 && m_b > 0;
  if (biv && both && N > ERPL_CMP_ENERGY_MAX_POINTS)
    return erpl_fail(ERPL_ERR_INVALID,
                     "the bivariate test pools %lld + %lld members, more than ERPL_CMP_ENERGY_MAX_POINTS = %d (its cost grows with "
                     "N^2 P): spec->row_x = -1 runs the rank tests alone",
                     (long long)m_a, (long long)m_b, ERPL_CMP_ENERGY_MAX_POINTS);

  const double nan = NAN;
  memset(result, 0, sizeof(*result));
  result->n_a = n_a; result->n_b = n_b; result->count_a = m_a; result->count_b = m_b;
  result->n_masked_a = (int64_t)h.counter[0][1]; result->n_masked_b = (int64_t)h.counter[1][1];
  result->n_non_finite_a = (int64_t)h.counter[0][2]; result->n_non_finite_b = (int64_t)h.counter[1][2];
  result->n_rows = R; result->n_q = nq; result->permutations = P; result->bivariate = biv && both ? 1 : 0;
  auto blank = [nan](erpl_cmp_test& t) { t.statistic = t.p_value = t.null_mean = t.null_hi = nan; t.exceed = 0; };
  for (int j = 0; j < ERPL_CMP_MAX_ROWS; ++j) {
    erpl_cmp_row& o = result->row[j];
    o.mean_a = o.std_a = o.mean_b = o.std_b = o.ks_at = o.prob_superiority = nan;
    for (int k = 0; k < ERPL_ANALYSIS_MAX_Q; ++k) o.quantile_a[k] = o.quantile_b[k] = o.shift[k] = nan;
    blank(o.ks); blank(o.mw); blank(o.cvm);
  }
  result->d_ab = result->d_aa = result->d_bb = nan;
  blank(result->energy);

  // per side: mean, std and quantiles, by the passes of erpl_mc_analyze over the side's samples with its population bytes
  // as the mask: the summary rows in one launch, `extra` as a one-row summary in a second
  int32_t est_rows[ERPL_CMP_MAX_ROWS];
  int est_of[ERPL_CMP_MAX_ROWS], n_est = 0, has_extra = 0;   // row j of the spec: rows[s][0].row[est_of[j]], or rows[s][1].row[0] (-1)
  for (int j = 0; j < R; ++j) {
    if (spec->rows[j] == ERPL_CMP_ROW_EXTRA) { est_of[j] = -1; has_extra = 1; }
    else { est_of[j] = n_est; est_rows[n_est++] = spec->rows[j]; }
  }
  for (int s = 0; s < 2; ++s) {
    if (n_est > 0) ERPL_TRY(describe_rows(c, summary_of[s], pop_of[s], n_of[s], est_rows, n_est, spec->q, nq, &h.rows[s][0], st));
    if (has_extra) ERPL_TRY(describe_rows(c, extra_of[s], pop_of[s], n_of[s], nullptr, 1, spec->q, nq, &h.rows[s][1], st));
  }
  auto finish_sides = [&]() {
    for (int j = 0; j < R; ++j) {
      erpl_row_stats sa, sb;
      finish_row_stats(est_of[j] < 0 ? h.rows[0][1].row[0] : h.rows[0][0].row[est_of[j]], spec->q, nq, true, sa);
      finish_row_stats(est_of[j] < 0 ? h.rows[1][1].row[0] : h.rows[1][0].row[est_of[j]], spec->q, nq, true, sb);
      erpl_cmp_row& o = result->row[j];
      o.mean_a = sa.mean; o.std_a = sa.std; o.mean_b = sb.mean; o.std_b = sb.std;
      for (int k = 0; k < nq; ++k) {
        o.quantile_a[k] = sa.quantile[k]; o.quantile_b[k] = sb.quantile[k];
        o.shift[k] = sb.quantile[k] - sa.quantile[k];
      }
    }
  };
  if (!both) {   // an empty side: counts, the other side's description, NaN elsewhere
    if (null_out) HIP_TRY(hipMemsetAsync(null_out, 0xff, 8 * n_null, st));   // the all-ones byte pattern is a NaN
    HIP_TRY(hipStreamSynchronize(st));
    finish_sides();
    return ERPL_OK;
  }

  size_t sort_bytes = 0;
  LAUNCH_TRY(erpl_boot_temp_bytes(N, &sort_bytes), "radix sort sizing failed");
  const ErplCompareLayout at = erpl_compare_layout(n_a, n_b, N, R, P, biv, select_bytes, sort_bytes);
  ERPL_TRY(c->cmp.grow(at.need));
  char* buf = c->cmp.buf;
  a.src_a = src_of[0]; a.src_b = src_of[1];
  for (int j = 0; j < R; ++j) {
    a.val[j] = (double*)(buf + at.val[j]);
    a.sidx[j] = (uint32_t*)(buf + at.sidx[j]);
    a.r2e[j] = (unsigned long long*)(buf + at.r2e[j]);
  }
  a.xy = (double*)(buf + at.xy);
  a.keys = (unsigned long long*)(buf + at.keys); a.idx = (uint32_t*)(buf + at.idx);
  a.temp = buf + at.temp; a.temp_bytes = at.temp_bytes;
  a.thr = (unsigned long long*)(buf + at.thr); a.bits = (unsigned long long*)(buf + at.bits);
  a.cnt = (uint32_t*)(buf + at.cnt); a.part = (ErplCmpRank*)(buf + at.part); a.rank = (ErplCmpRank*)(buf + at.rank);
  a.at_value = (double*)(buf + at.at_value); a.epart = (double*)(buf + at.epart); a.eout = (double*)(buf + at.eout);
  a.seed = spec->seed; a.N = (uint64_t)N; a.m_a = (uint64_t)m_a;
  a.n_rows = R; a.bivariate = biv ? 1 : 0; a.permutations = P; a.words = at.words; a.wb = at.wb;
  LAUNCH_TRY(erpl_launch_cmp_prepare(a, stream), "rank pass failed");
  for (int w0 = 0; w0 < at.words; w0 += at.wb)   // the permutations in blocks of wb words: the label bits of one block at a time
    KERNEL_TRY(erpl_launch_cmp_block(a, w0, std::min(at.wb, at.words - w0), stream));

  const size_t Q = (size_t)P + 1, all = (size_t)at.words * 64;
  std::vector<ErplCmpRank> rank((size_t)R * all);
  std::vector<double> eout(3 * all), at_value(R), null_host(n_null, nan), values(P), sorted;
  HIP_TRY(hipMemcpyAsync(rank.data(), a.rank, rank.size() * sizeof(ErplCmpRank), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(at_value.data(), a.at_value, R * sizeof(double), hipMemcpyDeviceToHost, st));
  if (biv) HIP_TRY(hipMemcpyAsync(eout.data(), a.eout, eout.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  finish_sides();

  const double da = (double)m_a, db = (double)m_b;
  const int64_t mm = m_a * m_b;   // < 2^62
  for (int j = 0; j < R; ++j) {
    const ErplCmpRank* rk = rank.data() + (size_t)j * all;
    erpl_cmp_row& o = result->row[j];
    auto u2 = [&](const ErplCmpRank& r) { return (int64_t)r.sum2r - m_a * (m_a + 1); };
    auto mw = [&](const ErplCmpRank& r) { const int64_t v = u2(r) - mm; return v < 0 ? -v : v; };
    o.ks_num = rk[0].k; o.u2_a = u2(rk[0]); o.ks_at = at_value[j]; o.ks_sign = (int32_t)rk[0].sign;
    o.prob_superiority = (double)o.u2_a / ((2.0 * da) * db);
    o.ks.statistic = (double)rk[0].k / (da * db);
    o.mw.statistic = (double)mw(rk[0]);
    o.cvm.statistic = cmp_cvm(rk[0], m_a, m_b);
    if (P == 0) continue;
    double* nk = null_host.data() + (size_t)(3 * j) * P;
    for (size_t q = 1; q < Q; ++q) {
      const double t = cmp_cvm(rk[q], m_a, m_b);
      nk[q - 1] = (double)rk[q].k; nk[P + q - 1] = (double)u2(rk[q]); nk[2 * (size_t)P + q - 1] = t;
      o.ks.exceed += rk[q].k >= rk[0].k ? 1 : 0;
      o.mw.exceed += mw(rk[q]) >= mw(rk[0]) ? 1 : 0;
      o.cvm.exceed += t >= o.cvm.statistic ? 1 : 0;
    }
    for (size_t q = 1; q < Q; ++q) values[q - 1] = (double)rk[q].k / (da * db);
    cmp_null(values, spec->level, sorted, o.ks);
    for (size_t q = 1; q < Q; ++q) values[q - 1] = (double)mw(rk[q]);
    cmp_null(values, spec->level, sorted, o.mw);
    values.assign(nk + 2 * (size_t)P, nk + 3 * (size_t)P);
    cmp_null(values, spec->level, sorted, o.cvm);
  }
  if (biv) {
    auto energy = [&](size_t q, double* aa, double* ab, double* bb) {
      *aa = eout[3 * q] / (da * da); *ab = eout[3 * q + 1] / (da * db); *bb = eout[3 * q + 2] / (db * db);
      return (2.0 * *ab - *aa) - *bb;
    };
    double aa, ab, bb;
    result->energy.statistic = energy(0, &result->d_aa, &result->d_ab, &result->d_bb);
    if (P > 0) {
      double* ne = null_host.data() + (size_t)(3 * R) * P;
      for (size_t q = 1; q < Q; ++q) {
        ne[q - 1] = energy(q, &aa, &ab, &bb);
        result->energy.exceed += ne[q - 1] >= result->energy.statistic ? 1 : 0;
      }
      values.assign(ne, ne + P);
      cmp_null(values, spec->level, sorted, result->energy);
    }
  }
  if (null_out) {
    HIP_TRY(hipMemcpyAsync(null_out, null_host.data(), 8 * n_null, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return ERPL_OK;
}

}  // extern "C"
