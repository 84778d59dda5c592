// fp64 correctness-gate instantiation (BASELINE config 2): reference operation order, IEEE
// division/sqrt, libm-grade transcendentals, FMA contraction off (see Makefile).
#define ERPL_FAITHFUL 1
#include "erpl_kernels.inc"
