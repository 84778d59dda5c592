// fp32 throughput instantiation (BASELINE configs 3-5): algebraic shortcuts + hardware
// transcendental instructions; time stays fp64.
#define ERPL_FAST_F32 1
#include "erpl_kernels.inc"
