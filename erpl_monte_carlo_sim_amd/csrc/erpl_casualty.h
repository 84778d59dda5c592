// erpl_casualty.h — the per-job rules of erpl_mc_casualty (include/erpl_mc.h), one definition for the device (erpl_casualty.hip)
// and the host (erpl_casualty.hip's own host half, erpl_casualty_check.cpp): which job is landed and lethal, its cell, the
// integer weights of the hazard map, the centres of the cells and the cut of the smoothing pass into slices.
// The cell is erpl_bin_of of erpl_tally.h over ErplEdges - the rule of erpl_mc_histogram_xy, not restated here.
// Every unit that includes it is built without FMA contraction.  Internal: never installed.
#pragma once
#include "erpl_tally.h"

#define ERPL_CAS_LANDED 1
#define ERPL_CAS_LETHAL 2
#define ERPL_CAS_Q_MOST 40
#define ERPL_CAS_Q_LEAST 16
// the smoothing pass: a workgroup owns ERPL_CAS_TILE cell centres and one slice of the rows; the rows are cut into slices
// until the launch has about ERPL_CAS_TARGET_BLOCKS workgroups
#define ERPL_CAS_TILE 1024
#ifndef ERPL_CAS_TARGET_BLOCKS
#define ERPL_CAS_TARGET_BLOCKS 1024   // measured against 256 and 4096: DESIGN.md 8.19
#endif

struct ErplCasRaster {
  double lo_x, hi_x, lo_y, hi_y;
  int32_t bins_x, bins_y;
};

// LANDED iff X, Y and VIMPACT are finite; LETHAL iff landed and (0.5 * mass) * (V * V) >= ke_min.  half_mass = 0.5 * mass.
ERPL_TALLY_HD int erpl_cas_class(double x, double y, double v, double half_mass, double ke_min) {
  if (!(erpl_is_finite(x) && erpl_is_finite(y) && erpl_is_finite(v))) return 0;
  return half_mass * (v * v) >= ke_min ? (ERPL_CAS_LANDED | ERPL_CAS_LETHAL) : ERPL_CAS_LANDED;
}

// the cell of a finite point: false off the raster, otherwise *cell = ix * bins_y + iy
ERPL_TALLY_HD bool erpl_cas_cell(const ErplCasRaster& g, const ErplEdges& ex, const ErplEdges& ey, double x, double y, int32_t* cell) {
  if (!(x >= g.lo_x && x <= g.hi_x && y >= g.lo_y && y <= g.hi_y)) return false;
  *cell = erpl_bin_of(x, g.lo_x, g.hi_x, g.bins_x, ex) * g.bins_y + erpl_bin_of(y, g.lo_y, g.hi_y, g.bins_y, ey);
  return true;
}

// the centre of cell i of an axis
ERPL_TALLY_HD double erpl_cas_centre(const ErplEdges& e, int i) { return 0.5 * (e[i] + e[i + 1]); }

ERPL_TALLY_HD double erpl_cas_cell_area(const ErplCasRaster& g) {
  return ((g.hi_x - g.lo_x) / (double)g.bins_x) * ((g.hi_y - g.lo_y) / (double)g.bins_y);
}

// Q = min(40, 62 - bit_length(m * n_nodes * n_fragments)): every cell takes all jobs at the largest weight without overflow
inline int erpl_cas_q(int64_t m, int32_t n_nodes, int32_t n_fragments) {
  uint64_t jobs = (uint64_t)m * (uint64_t)n_nodes * (uint64_t)n_fragments;
  int bits = 0;
  while (jobs) { ++bits; jobs >>= 1; }
  const int q = 62 - bits;
  return q < ERPL_CAS_Q_MOST ? q : ERPL_CAS_Q_MOST;
}

// W = floor((w / w_max) * 2^Q), 0 for w_max = 0
inline int64_t erpl_cas_weight(double w, double w_max, int q) {
  if (!(w_max > 0.0)) return 0;
  return (int64_t)floor((w / w_max) * ldexp(1.0, q));
}

// hazard[c] = (double)M[c] * erpl_cas_scale: 0 without a counted column
inline double erpl_cas_scale(double w_max, int q, int64_t m_c) { return m_c > 0 ? (w_max * ldexp(1.0, -q)) / (double)m_c : 0.0; }

// the rows of the smoothing pass per slice, a function of the shapes alone (rows, cells >= 1)
inline int erpl_cas_slices(int rows, int64_t cells, int* per_slice) {
  const int64_t blocks = (cells + ERPL_CAS_TILE - 1) / ERPL_CAS_TILE;
  const int64_t want = (ERPL_CAS_TARGET_BLOCKS + blocks - 1) / blocks, most = rows < want ? rows : want;
  const int per = (int)((rows + most - 1) / most);
  *per_slice = per;
  return (rows + per - 1) / per;
}

// One job on the host, for erpl_casualty_check: what it adds to the map (words [bins_x * bins_y]) and its hazard.
inline double erpl_cas_job_host(const ErplCasRaster& g, double x, double y, double v, double half_mass, double ke_min, double c_f,
                                int64_t weight, const double* population, int64_t* words, int* cls_out) {
  const int cls = erpl_cas_class(x, y, v, half_mass, ke_min);
  if (cls_out) *cls_out = cls;
  int32_t cell = 0;
  if (!(cls & ERPL_CAS_LETHAL) ||
      !erpl_cas_cell(g, erpl_edges_of(g.lo_x, g.hi_x, g.bins_x), erpl_edges_of(g.lo_y, g.hi_y, g.bins_y), x, y, &cell))
    return 0.0;
  words[cell] += weight;
  return c_f * population[cell];
}
