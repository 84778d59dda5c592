// erpl_design.h — the values of erpl_mc_design, one definition for the host (erpl_mc_design_host, erpl_design_check.cpp)
// and the device (erpl_design_fill in erpl_design.hip).  Internal: never installed.  The contract is in include/erpl_mc.h;
// in short, for row r (global), column i (global) of a design (seed, kind, n, block = m):
//   replicate   rho = i / m, local index l = i % m
//   round keys  Philox4x32-10, key (seed lo, seed hi), counters (r, 0, rho, 2) and (r, 1, rho, 2): k0..k3, then k4, k5
//   stratum     pi = perm(l): six Feistel rounds on 2 b bits (4^b >= m), walked until the value is below m
//   jitter      Philox counter (j lo, j hi, r, 1), j = i >> 1; even i: o0 | o1 << 32, odd i: o2 | o3 << 32;
//               u = ((draw >> 11) + 0.5) 2^-53
//   p           RANDOM u; LHS (pi + u) / m, kept below pi + 1; LHS_CENTRED (pi + 0.5) / m
//   normal rows Wichura's AS 241 PPND16 of p
// Permutation, jitter and p are integer work plus correctly rounded +, * by a power of two and /: the same bits on the host and
// on the device as long as the unit is built without FMA contraction.  PPND16 goes through log and sqrt of the platform.
#pragma once
#include <math.h>
#include <stdint.h>

#include "erpl_mc.h"
#include "erpl_philox.h"

#define ERPL_DESIGN_HD ERPL_PHILOX_HD
// trips of the cycle walk after which a value is given up (NaN and an error): see erpl_design_perm
#define ERPL_DESIGN_WALK_CAP 4096

struct ErplDesignKeys {
  uint32_t k[6];
};

ERPL_DESIGN_HD ErplDesignKeys erpl_design_keys(uint64_t seed, uint32_t row, uint32_t rep) {
  const ErplPhiloxOut a = erpl_philox4x32_10(row, 0u, rep, 2u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const ErplPhiloxOut b = erpl_philox4x32_10(row, 1u, rep, 2u, (uint32_t)seed, (uint32_t)(seed >> 32));
  ErplDesignKeys K;
  K.k[0] = a.w[0]; K.k[1] = a.w[1]; K.k[2] = a.w[2]; K.k[3] = a.w[3]; K.k[4] = b.w[0]; K.k[5] = b.w[1];
  return K;
}

// the MurmurHash3 finaliser
ERPL_DESIGN_HD uint32_t erpl_fmix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}

// b: the smallest integer >= 1 with 4^b >= m (m < 2^31: b <= 16, and a walked value fits 32 bits)
ERPL_DESIGN_HD uint32_t erpl_design_half_bits(uint32_t m) {
  uint32_t b = 1;
  while (b < 16 && ((uint32_t)1 << (2 * b)) < m) ++b;
  return b;
}

// pi = perm(l) over [0, m), l < m.  The six rounds are a bijection F of [0, 4^b) whatever the round function is, so the walk
// l, F(l), F(F(l)), .. runs along the cycle of F through l and comes back to l < m: it ends after at most 4^b - m + 1 trips,
// which is below the cap for b <= 6.  For larger b more than a quarter of the domain lies below m, and a network whose rounds
// mix lands there with that probability on every trip: 4096 misses in a row have probability below (3/4)^4096 < 1e-511.  Only a
// coding slip in the rounds (one that makes F no bijection, or the mask wrong) can reach the cap; then `*capped` is set and the
// value is 0, so that no wave spins on it.
ERPL_DESIGN_HD uint32_t erpl_design_perm(const uint32_t* k, uint32_t b, uint32_t m, uint32_t l, bool* capped) {
  const uint32_t M = ((uint32_t)1 << b) - 1u;
  uint32_t x = l;
  for (int trip = 0; trip < ERPL_DESIGN_WALK_CAP; ++trip) {
    uint32_t L = x >> b, R = x & M;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const uint32_t t = L ^ (erpl_fmix32(R + k[r]) & M);
      L = R; R = t;
    }
    x = (L << b) | R;
    if (x < m) return x;
  }
  *capped = true;
  return 0u;
}

// u of GLOBAL column i of row `row`, in (0, 1)
ERPL_DESIGN_HD double erpl_design_jitter(uint64_t seed, uint32_t row, uint64_t i) {
  const uint64_t j = i >> 1;
  const ErplPhiloxOut o = erpl_philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), row, 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t draw = (i & 1) ? ((uint64_t)o.w[2] | ((uint64_t)o.w[3] << 32)) : ((uint64_t)o.w[0] | ((uint64_t)o.w[1] << 32));
  return ((double)(draw >> 11) + 0.5) * 0x1p-53;
}

// the double just below t, for t >= 1
ERPL_DESIGN_HD double erpl_design_below(double t) {
  uint64_t bits;
  __builtin_memcpy(&bits, &t, sizeof bits);
  --bits;
  __builtin_memcpy(&t, &bits, sizeof bits);
  return t;
}

// p of a stratum and a jitter: in [pi / m, (pi + 1) / m) and strictly inside (0, 1)
ERPL_DESIGN_HD double erpl_design_p(int kind, uint32_t pi, double u, uint32_t m) {
  if (kind == ERPL_DESIGN_RANDOM) return u >= 1.0 ? erpl_design_below(1.0) : u;   // u = 1: draw >> 11 = 2^53 - 1, rounded up by the + 0.5
  if (kind == ERPL_DESIGN_LHS_CENTRED) return ((double)pi + 0.5) / (double)m;
  const double top = (double)pi + 1.0;
  double s = (double)pi + u;
  if (s >= top) s = erpl_design_below(top);
  return s / (double)m;
}

// sum of c[j] x^j, j = 0..7, by Horner
ERPL_DESIGN_HD double erpl_design_poly7(const double* c, double x) {
  double s = c[7];
#pragma unroll
  for (int j = 6; j >= 0; --j) s = s * x + c[j];
  return s;
}

// Wichura, Algorithm AS 241 (Applied Statistics 37, 1988), PPND16: the normal quantile of p in (0, 1)
ERPL_DESIGN_HD double erpl_design_ppnd16(double p) {
  const double A[8] = {3.3871328727963666080e0, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
                       4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3};
  const double B[8] = {1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3,
                       2.1213794301586595867e4, 3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3};
  const double Cc[8] = {1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
                        1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4};
  const double D[8] = {1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1,
                       1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9};
  const double E[8] = {6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
                       2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7};
  const double F[8] = {1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
                       7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15};
  // one quotient num / den for every branch: a wave whose lanes take different branches divides once (-(C / D) = (-C) / D)
  const double q = p - 0.5;
  double num, den;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    num = q * erpl_design_poly7(A, r);
    den = erpl_design_poly7(B, r);
  } else {
    double r = sqrt(-log(q < 0.0 ? p : 1.0 - p));
    if (r <= 5.0) {
      r -= 1.6;
      num = erpl_design_poly7(Cc, r);
      den = erpl_design_poly7(D, r);
    } else {
      r -= 5.0;
      num = erpl_design_poly7(E, r);
      den = erpl_design_poly7(F, r);
    }
    if (q < 0.0) num = -num;
  }
  return num / den;
}

// The value of row `row`, column i: k the round keys of (row, i / m), l = i % m, b = erpl_design_half_bits(m).  NaN (and
// *capped) where the walk gave up.
ERPL_DESIGN_HD double erpl_design_value(uint64_t seed, int kind, bool normal, uint32_t row, uint64_t i, const uint32_t* k,
                                        uint32_t b, uint32_t m, uint32_t l, bool* capped) {
  bool cap = false;
  const uint32_t pi = kind == ERPL_DESIGN_RANDOM ? 0u : erpl_design_perm(k, b, m, l, &cap);
  if (cap) { *capped = true; return (double)NAN; }
  const double u = kind == ERPL_DESIGN_LHS_CENTRED ? 0.0 : erpl_design_jitter(seed, row, i);
  const double p = erpl_design_p(kind, pi, u, m);
  return normal ? erpl_design_ppnd16(p) : p;
}
