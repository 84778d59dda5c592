// erpl_philox.h — the draws of erpl_mc_bootstrap, erpl_mc_sobol and erpl_mc_compare, one definition for the host
// (erpl_mc_bootstrap_indices, erpl_mc_compare_labels) and the device (erpl_boot_replicate in erpl_bootstrap.hip,
// erpl_sobol_replicate in erpl_sobol.hip, the label passes of erpl_compare.hip).  Internal: never installed.
//
// The generator is Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011):
// ten rounds of two 32 x 32 -> 64 bit multiplies (0xD2511F53, 0xCD9E8D57), the key bumped by (0x9E3779B9, 0xBB67AE85)
// between rounds.  The draw contract of include/erpl_mc.h on top of it:
//   key      (seed & 0xffffffff, seed >> 32)
//   counter  (j & 0xffffffff, j >> 32, b, 0): b the replicate, j the index of a PAIR of draws
//   words    o0..o3 -> A = o0 | o1 << 32 (draw 2j), B = o2 | o3 << 32 (draw 2j + 1)
//   index    (u * m) >> 64 of a 64-bit draw u: a dense population index below m, bias at most m / 2^64
//   label    erpl_mc_compare: the key of pooled member i in permutation p is draw i of replicate p; side A is the m_a members
//            with the smallest (key, i) pairs.  With (thr_key, thr_idx) the m_a-th smallest pair, the label is one comparison.
// Counter word 3 is a TAG that keeps the families apart: 0 the bootstrap family above, 1 the jitter and 2 the round keys of
// erpl_mc_design (erpl_design.h), 3 the proposals of erpl_mc_subset_propose (erpl_subset.h), 4 the scramble keys
// of erpl_mc_qmc (erpl_qmc.h), 5 the break-up directions of erpl_mc_debris (erpl_debris.h).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ERPL_PHILOX_HD __host__ __device__ __forceinline__
#else
#define ERPL_PHILOX_HD inline
#endif

struct ErplPhiloxOut {
  uint32_t w[4];
};

ERPL_PHILOX_HD ErplPhiloxOut erpl_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  ErplPhiloxOut o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// the two 64-bit draws of pair j of replicate b
ERPL_PHILOX_HD void erpl_boot_pair(uint64_t seed, uint32_t b, uint64_t j, uint64_t* A, uint64_t* B) {
  const ErplPhiloxOut o = erpl_philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), b, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  *A = (uint64_t)o.w[0] | ((uint64_t)o.w[1] << 32);
  *B = (uint64_t)o.w[2] | ((uint64_t)o.w[3] << 32);
}

// (u * m) >> 64
ERPL_PHILOX_HD uint64_t erpl_boot_index(uint64_t u, uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(u, m);
#else
  return (uint64_t)(((unsigned __int128)u * m) >> 64);
#endif
}

// the 64-bit draw t of replicate b
ERPL_PHILOX_HD uint64_t erpl_boot_draw(uint64_t seed, uint32_t b, uint64_t t) {
  uint64_t A, B;
  erpl_boot_pair(seed, b, t >> 1, &A, &B);
  return (t & 1) ? B : A;
}

// erpl_mc_compare: is the pooled member i with the key `key` on side A, (thr_key, thr_idx) being the m_a-th smallest pair?
ERPL_PHILOX_HD bool erpl_cmp_label(uint64_t key, uint64_t i, uint64_t thr_key, uint64_t thr_idx) {
  return key < thr_key || (key == thr_key && i <= thr_idx);
}
