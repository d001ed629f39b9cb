#!/bin/bash
# build a comparison library with extra defines on conp_zn.hip and conp_kernels.hip (the product's other objects as they are: build
# the product first; the object list is csrc/Makefile's):
# bash tools/build_variant.sh NAME "-DZN_TIMELINE" (or "-DSYM_TIMELINE") -> conp_amd/libconp_hip_NAME.so
set -e
C=$(dirname "$0")/../lammps-user-conp2_amd/csrc
OBJS=""
for f in $(make -s -C "$C" print-objs); do
  case $f in
    conp_zn|conp_kernels)
      /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $2 -c $C/$f.hip -o $C/${f}_var_$1.o
      OBJS="$OBJS $C/${f}_var_$1.o" ;;
    *) OBJS="$OBJS $C/$f.o" ;;
  esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $C/../conp_amd/libconp_hip_$1.so $OBJS
