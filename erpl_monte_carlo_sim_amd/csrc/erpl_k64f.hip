// fp64 throughput instantiation (ERPL_PREC_F64_FAST): the short formulation of the fp32 RHS
// (one reciprocal per denominator, interval-record atmosphere, no trig of atan2) carried in double
// with FMA contraction.  MI355X runs fp64 vector FMAs at half the fp32 rate, so this build keeps
// fp64 parity with the reference on the chaotic samples at a fraction of the cost
// of the reference-order gate kernel (erpl_k64.hip).  Round 3: two waves per SIMD (<= 256 registers
// per lane: lane state, wind interval and table records in LDS - note [1] of erpl_k_config.h).
// Round 4: lanes whose speed passes 1e6 m/s are handed to the reference-order kernel (note [2]): which
// intermediate of a blow-up's last steps turns inf and which NaN decides how the reference's flight ends, and only
// the reference's own operation order reproduces that.
#define ERPL_FAST_F64 1
#include "erpl_kernels.inc"
