#!/bin/bash
# experimental liboi variants for timing A/B (tools only, never shipped):
#   build_exp/liboi_<tag>.so built with extra -D flags on oi_kernels.hip,
#   linked with every other object of the in-tree build (run make first)
# usage: scripts/build_exp_lib.sh <tag> "<-DFLAGS>"
set -e
cd "$(dirname "$0")/../optimalinterpolation_amd"
mkdir -p ../build_exp
/opt/rocm/bin/hipcc -O3 -std=c++20 -fPIC --offload-arch=gfx950 -ffp-contract=fast $2 -c csrc/oi_kernels.hip -o ../build_exp/oi_kernels_$1.o
others=$(ls build/*.o | grep -v '/oi_kernels\.o$')
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o ../build_exp/liboi_$1.so ../build_exp/oi_kernels_$1.o $others
