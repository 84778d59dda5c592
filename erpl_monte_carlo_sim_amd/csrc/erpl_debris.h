// erpl_debris.h — the rules of erpl_mc_debris (include/erpl_mc.h) that exist once: the break-up direction of a fragment, the
// step rule of its fall and the tick count of its fall time.  One definition for the host (erpl_mc_debris_directions_host,
// erpl_debris_check.cpp) and the device (erpl_k_debris.h in the gate unit).  Internal: never installed.  Every unit that
// includes it is built without FMA contraction: every operation named below rounds once, on its own.
//
// THE CONTRACT
// Direction  of (seed, sample id, node k, fragment f), by Marsaglia's rejection method (Ann. Math. Stat. 43, 1972): try
//            t = 0, 1, .. 15 draws one Philox4x32-10 block under erpl_philox.h's contract - key (seed & 0xffffffff,
//            seed >> 32), counter (id & 0xffffffff, id >> 32, (t << 18) | (k << 6) | f, ERPL_DEBRIS_PHILOX_TAG) - and reads
//            A = o0 | o1 << 32, B = o2 | o3 << 32;  a = ((double)(A >> 12) + 0.5) * 2^-51 - 1.0 (exact: an odd multiple of
//            2^-52 in (-1, 1)), b likewise from B.  s = a * a + b * b; the first try with s < 1.0 is accepted:
//            q = sqrt(1.0 - s), d = ((2.0 * a) * q, (2.0 * b) * q, 1.0 - 2.0 * s).  No try accepted: d = (0, 0, 1).
//            +, -, *, sqrt alone, each correctly rounded on both sides: the host and the device give the same bits.
// Step rule  k0 = the drag rate ((0.5 * rho) * vn) / beta of the step's own k1 evaluation; m = the smallest integer in
//            0 .. ERPL_DEBRIS_MAX_HALVINGS with k0 * (dt * 2^-m) <= stiff_limit, ERPL_DEBRIS_MAX_HALVINGS if there is none (a
//            NaN k0 too).  The step is h = dt * 2^-m, its half (0.5 * dt) * 2^-m and its sixth (dt / 6.0) * 2^-m: scaling by a
//            power of two is exact, so m = 0 gives the three constants of a fixed-step fall to the bit.
// Ticks      time is counted in units of dt * 2^-16: a step with m halvings adds 2^(16 - m) ticks, and a crossing at the
//            fraction wq of such a step gives TFALL = ((double)ticks + wq * 2^(16 - m)) * (dt * 2^-16) - with m = 0
//            throughout, (n + wq) * dt to the bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "erpl_philox.h"

#define ERPL_DEBRIS_HD ERPL_PHILOX_HD

#define ERPL_DEBRIS_PHILOX_TAG 5u   // counter word 3 (the list of tags: erpl_philox.h)
#define ERPL_DEBRIS_MAX_TRIES 16
#define ERPL_DEBRIS_TICK_BITS 16    // = ERPL_DEBRIS_MAX_HALVINGS of include/erpl_mc.h

// a uniform in (-1, 1) from a 64-bit draw: an odd multiple of 2^-52, never -1, 0 or 1
ERPL_DEBRIS_HD double erpl_debris_uniform(uint64_t u) { return ((double)(u >> 12) + 0.5) * 0x1p-51 - 1.0; }

// the pairs (a, b) of the tries of one (seed, sample id, node, fragment)
struct ErplDebrisPhilox {
  uint64_t seed, id;
  uint32_t node, fragment;
  ERPL_DEBRIS_HD void operator()(uint32_t t, double* a, double* b) const {
    const ErplPhiloxOut o = erpl_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), (t << 18) | (node << 6) | fragment,
                                               ERPL_DEBRIS_PHILOX_TAG, (uint32_t)seed, (uint32_t)(seed >> 32));
    *a = erpl_debris_uniform((uint64_t)o.w[0] | ((uint64_t)o.w[1] << 32));
    *b = erpl_debris_uniform((uint64_t)o.w[2] | ((uint64_t)o.w[3] << 32));
  }
};

// Marsaglia's method over any source of pairs: pairs(t, &a, &b) gives try t.  The source is a parameter so that the host
// check can reach the fallback after ERPL_DEBRIS_MAX_TRIES rejections with a source that never lands in the disc (the test
// hook of erpl_debris_check.cpp; a seed whose sixteen Philox tries all miss has probability 0.2146^16 = 2e-11).
// Returns the number of tries made.
template <class Pairs>
ERPL_DEBRIS_HD int erpl_debris_direction_from(const Pairs& pairs, double* d) {
  for (uint32_t t = 0; t < ERPL_DEBRIS_MAX_TRIES; ++t) {
    double a, b;
    pairs(t, &a, &b);
    const double aa = a * a, bb = b * b;
    const double s = aa + bb;
    if (s < 1.0) {
      const double r = 1.0 - s;
      const double q = sqrt(r);
      d[0] = (2.0 * a) * q; d[1] = (2.0 * b) * q; d[2] = 1.0 - 2.0 * s;
      return (int)t + 1;
    }
  }
  d[0] = 0.0; d[1] = 0.0; d[2] = 1.0;
  return ERPL_DEBRIS_MAX_TRIES;
}

ERPL_DEBRIS_HD void erpl_debris_direction(uint64_t seed, uint64_t id, uint32_t node, uint32_t fragment, double* d) {
  ErplDebrisPhilox p;
  p.seed = seed; p.id = id; p.node = node; p.fragment = fragment;
  (void)erpl_debris_direction_from(p, d);
}

// the step rule: m of a drag rate k0; *scale = 2^-m
ERPL_DEBRIS_HD int erpl_debris_halvings(double k0, double dt, double stiff_limit, double* scale) {
  int m = 0;
  double sc = 1.0;
  while (m < ERPL_DEBRIS_TICK_BITS && !(k0 * (dt * sc) <= stiff_limit)) { sc = sc * 0.5; ++m; }
  *scale = sc;
  return m;
}

// the ticks of one step with m halvings
ERPL_DEBRIS_HD int64_t erpl_debris_step_ticks(int m) { return (int64_t)1 << (ERPL_DEBRIS_TICK_BITS - m); }

// TFALL of a crossing at the fraction wq of a step with m halvings that began at `ticks`
ERPL_DEBRIS_HD double erpl_debris_tfall(int64_t ticks, double wq, int m, double dt) {
  return ((double)ticks + wq * (double)erpl_debris_step_ticks(m)) * (dt * 0x1p-16);
}
