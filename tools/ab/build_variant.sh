#!/bin/bash
# usage: build_variant.sh <tag> [-nosched] [extra flags for the fp64 throughput unit]  ->  tools/ab/liberpl_mc_<tag>.so
# (A/B experiment builds of the library; loaded through ERPL_LIB, never shipped)
# The unit's flags are the Makefile's (`make -s flags-k64f`); -nosched drops its scheduler strategy.
set -e
cd "$(dirname "$0")/../../erpl_monte_carlo_sim_amd/csrc"
T=$1; shift
MK=(); ARGS=()
for a in "$@"; do if [ "$a" = "-nosched" ]; then MK+=("F64FSCHED="); else ARGS+=("$a"); fi; done
FL=$(make -s flags-k64f "${MK[@]}")
# the product's own objects (the Makefile's list, built if they are not there) with the variant of the fp64 throughput unit
OBJS=$(make -s objs)
make -s $OBJS
/opt/rocm/bin/hipcc $FL "${ARGS[@]}" -c erpl_k64f.hip -o /tmp/k64f_$T.o 2>/dev/null
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/ab/liberpl_mc_$T.so ${OBJS/erpl_k64f.o//tmp/k64f_$T.o} -lpthread
echo built tools/ab/liberpl_mc_$T.so
