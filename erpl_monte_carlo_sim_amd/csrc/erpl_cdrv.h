// erpl_cdrv.h — the host rules of erpl_mc_corridor_drivers (include/erpl_mc.h) and the standardised regression it shares with
// erpl_mc_correlation: pure functions, no HIP, so that erpl_cdrv_check.cpp drives them on tables before a kernel runs anywhere.
//   erpl_regress            R_ff beta = r_fy by Cholesky over the non-constant factors: THE one definition, for
//                           erpl_mc_correlation (all its rows at once) and erpl_mc_corridor_drivers (row by row, R = 1)
//   erpl_cdrv_row_view      where the sums of one row lie in the record the product pass hands back (erpl_stat_layout.h)
//   erpl_cdrv_centred       S_ab = sum a b - (sum a)(sum b) / count
//   erpl_cdrv_ambiguous     whether the sums alone decide that a factor is NOT constant over a row's population
//   erpl_cdrv_finish_row    sums -> pearson / src / r2 / pivot_min / regression_ok of one row
// Internal, never installed.  Compiled without FMA contraction wherever it is included.
#pragma once
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "erpl_stat_layout.h"

// Standardised regression of every non-constant row on the non-constant factors: R_ff beta = r_fy by Cholesky.  corr is the
// V x V correlation matrix (row-major) of the F factors followed by the R rows, constant[v] marks a constant variable.  The
// k-th pivot is 1 - R^2 of factor k on the factors before it.  false: a pivot below 1e-10 or not finite (everything stays as
// it was).  pivot_min (optional): the smallest pivot met, the failing one included; NaN when no factor is in use.
inline bool erpl_regress(const double* corr, int V, int F, int R, const int32_t* constant, double (*coef)[ERPL_CORR_MAX_FACTORS],
                         double* r2, double* pivot_min = nullptr) {
  int use[ERPL_CORR_MAX_FACTORS], m = 0;
  for (int f = 0; f < F; ++f) if (!constant[f]) use[m++] = f;
  static thread_local double L[ERPL_CORR_MAX_FACTORS][ERPL_CORR_MAX_FACTORS];
  if (pivot_min) *pivot_min = NAN;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = corr[(size_t)use[i] * V + use[j]];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (pivot_min && !(*pivot_min <= s)) *pivot_min = s;   // a NaN pivot stays
        if (!(s >= 1e-10) || !std::isfinite(s)) return false;
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  for (int j = 0; j < R; ++j) {
    if (constant[F + j]) continue;
    double y[ERPL_CORR_MAX_FACTORS], beta[ERPL_CORR_MAX_FACTORS];
    for (int i = 0; i < m; ++i) {
      double s = corr[(size_t)(F + j) * V + use[i]];
      for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
    for (int i = m - 1; i >= 0; --i) {
      double s = y[i];
      for (int k = i + 1; k < m; ++k) s -= L[k][i] * beta[k];
      beta[i] = s / L[i][i];
    }
    double fit = 0.0;
    for (int i = 0; i < m; ++i) {
      coef[j][use[i]] = beta[i];
      fit += beta[i] * corr[(size_t)(F + j) * V + use[i]];
    }
    r2[j] = fit;
  }
  return true;
}

// The sums of one row in its record of erpl_cdrv_row_doubles(F, regression) doubles: with m the 0/1 membership of the row's
// population, x'_f the factors standardised over the base population and y' the row standardised over its own,
//   a[f] = sum m x'_f    n1 = sum m (the count again)    c[p] = sum m x'_f x'_g at p = erpl_cdrv_product_index(F, f, g)
//   b[f] = sum m y' x'_f sy = sum m y'                   syy = sum m y'^2
struct ErplCdrvRowView {
  const double* a;
  const double* c;
  const double* b;
  double n1, sy, syy;
};
inline ErplCdrvRowView erpl_cdrv_row_view(const double* rec, int F, bool regression) {
  const int nc = 16 * erpl_cdrv_product_blocks(F, regression);
  ErplCdrvRowView v;
  v.a = rec;
  v.n1 = rec[ERPL_CDRV_ONE];
  v.c = rec + ERPL_CDRV_LIN;
  v.b = rec + ERPL_CDRV_LIN + nc;
  v.sy = v.b[ERPL_CDRV_ONE];
  v.syy = rec[2 * ERPL_CDRV_LIN + nc];
  return v;
}

inline double erpl_cdrv_centred(double sab, double sa, double sb, double count) { return sab - sa * sb / count; }

// A factor that is constant over the population has S_xx = 0 up to the rounding of its two sums, at most 3 count 2^-53 of
// sum x'^2 however the sums are ordered (count < 2^31: below 7e-7).  S_xx above 1e-6 sum x'^2 therefore PROVES that the factor
// is not constant there; anything else is ambiguous and decided by the factor's exact extremes over the population.
inline bool erpl_cdrv_ambiguous(double sxx_raw, double sx, double count) {
  return !(erpl_cdrv_centred(sxx_raw, sx, sx, count) > 1e-6 * sxx_raw);
}

// pearson[F], src[F] (NULL without the regression), *r2, *pivot_min, *ok of one row from its sums (include/erpl_mc.h states
// the rules).  count: the row's population; row_constant: min == max of the row there; fconst[f]: factor f is constant there.
inline void erpl_cdrv_finish_row(int F, bool regression, int64_t count, bool row_constant, const int32_t* fconst,
                                 const ErplCdrvRowView& s, double* pearson, double* src, double* r2, double* pivot_min, int32_t* ok) {
  const double nan = NAN;
  for (int f = 0; f < F; ++f) {
    pearson[f] = nan;
    if (src) src[f] = nan;
  }
  *r2 = *pivot_min = nan;
  *ok = 0;
  if (count < 2) return;
  const double n = (double)count;
  const double syy = erpl_cdrv_centred(s.syy, s.sy, s.sy, n);
  double sxx[ERPL_CORR_MAX_FACTORS];
  for (int f = 0; f < F; ++f) {
    sxx[f] = erpl_cdrv_centred(s.c[f], s.a[f], s.a[f], n);
    if (!row_constant && !fconst[f]) pearson[f] = erpl_cdrv_centred(s.b[f], s.a[f], s.sy, n) / (sqrt(sxx[f]) * sqrt(syy));
  }
  if (!regression) return;
  // the correlation matrix of (factors, row) over the row's population, as erpl_regress reads it
  const int V = F + 1;
  static thread_local std::vector<double> corr;
  corr.assign((size_t)V * V, nan);
  int32_t constant[ERPL_CORR_MAX_FACTORS + 1];
  for (int f = 0; f < F; ++f) constant[f] = fconst[f];
  constant[F] = row_constant ? 1 : 0;
  for (int f = 0; f < F; ++f) {
    if (fconst[f]) continue;
    corr[(size_t)f * V + f] = 1.0;
    for (int g = f + 1; g < F; ++g) {
      if (fconst[g]) continue;
      const double sfg = erpl_cdrv_centred(s.c[erpl_cdrv_product_index(F, f, g)], s.a[f], s.a[g], n);
      corr[(size_t)f * V + g] = corr[(size_t)g * V + f] = sfg / (sqrt(sxx[f]) * sqrt(sxx[g]));
    }
    corr[(size_t)F * V + f] = corr[(size_t)f * V + F] = pearson[f];
  }
  double coef[1][ERPL_CORR_MAX_FACTORS], fit = nan;
  for (int f = 0; f < ERPL_CORR_MAX_FACTORS; ++f) coef[0][f] = nan;
  const bool held = erpl_regress(corr.data(), V, F, 1, constant, coef, &fit, pivot_min);
  *ok = held ? 1 : 0;
  if (!held || row_constant) return;
  for (int f = 0; f < F; ++f) src[f] = coef[0][f];
  *r2 = fit;
}
