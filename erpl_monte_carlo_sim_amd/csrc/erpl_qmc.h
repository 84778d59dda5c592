// erpl_qmc.h — the values of erpl_mc_qmc, one definition for the host (erpl_mc_qmc_host, erpl_qmc_check.cpp) and the device
// (erpl_qmc_fill in erpl_qmc.hip).  Internal: never installed.  The contract is in include/erpl_mc.h; in short, for row r
// (global), column i (global) of a design (seed, n, block = m, scramble, pad) on the dimension d = dims[r]:
//   replicate   rho = i / m, local index l = i % m
//   raw point   x = XOR over the set bits j of l (j = 0..30) of V[d][j]: direct binary order, V the Joe-Kuo direction numbers
//   keys        Philox4x32-10, key (seed lo, seed hi), counter (r, 0, rho, 4): k0, k1 its words 0 and 1
//   OWEN        bit k of x (k = 0..31 from the top) is flipped by fmix32(fmix32(s_k + k0) ^ k1) >> 31,
//               s_k = (1 << k) | (x >> (32 - k)): the k bits of the UNSCRAMBLED x above it, under a sentinel bit
//   p           OWEN ((double)x' + u) 2^-32, u the jitter of erpl_design.h, kept below x' + 1; RAW (x + 0.5) 2^-32
//   normal rows Wichura's AS 241 PPND16 of p (erpl_design.h)
//   pad rows    d = -1: erpl_design_value of (seed, pad, n, block, r, i), what erpl_mc_design writes
// Every loop has fixed bounds.  Integer work plus one exact conversion, one correctly rounded + and one product by a power of
// two: the same bits on the host and on the device as long as the unit is built without FMA contraction.
#pragma once
#include "erpl_design.h"

// counter word 3 of the scramble keys (erpl_philox.h lists the families)
#define ERPL_QMC_TAG 4u
#define ERPL_QMC_BITS 32

// The table: per dimension 1 .. ERPL_QMC_MAX_DIMS - 1 the primitive polynomial (its bit length less one is the degree s) and
// m_1 .. m_s.  A host array; the device reads the expanded V.
static const uint16_t kErplQmcTable[] = {
#include "erpl_qmc_table.inc"
};

// V[ERPL_QMC_MAX_DIMS][32]: V[d][j] = m_{j+1} 2^(31 - j), with m_k for k > s from the recurrence of Bratley and Fox
// (Algorithm 659): m_k = 2 a_1 m_{k-1} ^ 4 a_2 m_{k-2} ^ .. ^ 2^(s-1) a_{s-1} m_{k-s+1} ^ 2^s m_{k-s} ^ m_{k-s}.  Returns
// false where the table does not hold exactly the dimensions it should.
inline bool erpl_qmc_expand(uint32_t* V) {
  const size_t words = sizeof kErplQmcTable / sizeof kErplQmcTable[0];
  size_t at = 0;
  for (int j = 0; j < ERPL_QMC_BITS; ++j) V[j] = (uint32_t)1 << (31 - j);
  for (int d = 1; d < ERPL_QMC_MAX_DIMS; ++d) {
    if (at >= words) return false;
    const uint32_t poly = kErplQmcTable[at++];
    int s = 0;
    while ((poly >> (s + 1)) != 0) ++s;
    if (s < 1 || s > 13 || at + (size_t)s > words) return false;
    uint64_t m[ERPL_QMC_BITS];
    for (int j = 0; j < s; ++j) m[j] = kErplQmcTable[at++];
    for (int j = s; j < ERPL_QMC_BITS; ++j) {
      uint64_t v = m[j - s] ^ (m[j - s] << s);
      for (int k = 1; k < s; ++k)
        if ((poly >> (s - k)) & 1u) v ^= m[j - k] << k;
      m[j] = v;                                          // m_k < 2^k: below 2^32 here
    }
    for (int j = 0; j < ERPL_QMC_BITS; ++j) V[d * ERPL_QMC_BITS + j] = (uint32_t)(m[j] << (31 - j));
  }
  return at == words;
}

// x of the local index l < 2^31 from the 32 direction words of the row's dimension
ERPL_DESIGN_HD uint32_t erpl_qmc_raw(const uint32_t* v, uint32_t l) {
  uint32_t x = 0;
#pragma unroll
  for (int j = 0; j < 31; ++j) x ^= (0u - ((l >> j) & 1u)) & v[j];
  return x;
}

ERPL_DESIGN_HD void erpl_qmc_keys(uint64_t seed, uint32_t row, uint32_t rep, uint32_t* k0, uint32_t* k1) {
  const ErplPhiloxOut o = erpl_philox4x32_10(row, 0u, rep, ERPL_QMC_TAG, (uint32_t)seed, (uint32_t)(seed >> 32));
  *k0 = o.w[0]; *k1 = o.w[1];
}

// The nested uniform scramble of x under (k0, k1), lazily: the flip of a bit is a keyed hash of the bits above it, so every
// node of the binary tree of prefixes has its own fair coin and no coin is ever stored.
ERPL_DESIGN_HD uint32_t erpl_qmc_owen(uint32_t x, uint32_t k0, uint32_t k1) {
  uint32_t flips = 0;
#pragma unroll
  for (int k = 0; k < ERPL_QMC_BITS; ++k) {
    const uint32_t s = ((uint32_t)1 << k) | (k ? x >> (32 - k) : 0u);
    flips = (flips << 1) | (erpl_fmix32(erpl_fmix32(s + k0) ^ k1) >> 31);
  }
  return x ^ flips;
}

// p of a scrambled point and a jitter: in [x 2^-32, (x + 1) 2^-32) and strictly inside (0, 1)
ERPL_DESIGN_HD double erpl_qmc_p(uint32_t x, double u) {
  const double top = (double)x + 1.0;
  double s = (double)x + u;
  if (s >= top) s = erpl_design_below(top);
  return s * 0x1p-32;
}

// The value of a row on dimension d >= 0 with the direction words v: l = i % m, (k0, k1) the keys of (row, i / m).
ERPL_DESIGN_HD double erpl_qmc_value(uint64_t seed, int scramble, bool normal, uint32_t row, uint64_t i, const uint32_t* v,
                                     uint32_t l, uint32_t k0, uint32_t k1) {
  const uint32_t x = erpl_qmc_raw(v, l);
  double p;
  if (scramble == ERPL_QMC_RAW) p = ((double)x + 0.5) * 0x1p-32;
  else p = erpl_qmc_p(erpl_qmc_owen(x, k0, k1), erpl_design_jitter(seed, row, i));
  return normal ? erpl_design_ppnd16(p) : p;
}
