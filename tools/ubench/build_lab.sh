#!/bin/bash
# builds tools/ubench/mlp_lab against a diagnostic build of the two projection units (stamps on; DEFS= for none); run from the repo root.
# The staged-order weight images come from the library's own pack_net_image (handle.cpp): build the library first.
set -e
DEFS=${DEFS--DGBNNS_NET_STAMPS}
OUT=${OUT:-tools/ubench/mlp_lab}
OBJ=${OBJ:-/tmp/lab_build}
HIPFLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function $DEFS $EXTRA"
mkdir -p $OBJ
/opt/rocm/bin/hipcc $HIPFLAGS -c gbnns_dim_red_amd/csrc/mlp_net.hip -o $OBJ/mlp_net.o &
/opt/rocm/bin/hipcc $HIPFLAGS -c gbnns_dim_red_amd/csrc/mlp.hip -o $OBJ/mlp.o &
wait
LIBDIR=$(cd gbnns_dim_red_amd/lib && pwd)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -x hip -Igbnns_dim_red_amd/csrc tools/ubench/mlp_lab.cpp -x none $OBJ/mlp.o $OBJ/mlp_net.o \
    -L$LIBDIR -lgbnns_hip -Wl,-rpath,'$ORIGIN/../../gbnns_dim_red_amd/lib' -o $OUT
