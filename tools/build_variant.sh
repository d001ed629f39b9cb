#!/bin/bash
# build a comparison library with extra defines on conp_zn.hip and conp_kernels.hip (the product's other objects as they are):
# bash tools/build_variant.sh NAME "-DZN_TIMELINE" (or "-DSYM_TIMELINE") -> conp_amd/libconp_hip_NAME.so
set -e
C=$(dirname "$0")/../lammps-user-conp2_amd/csrc
for f in conp_zn conp_kernels; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $2 -c $C/$f.hip -o $C/${f}_var_$1.o
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $C/../conp_amd/libconp_hip_$1.so $C/conp_kernels_var_$1.o $C/conp_inverse.o $C/conp_pppm.o \
  $C/conp_rows.o $C/conp_tables.o $C/conp_zn_var_$1.o $C/conp_potential.o $C/conp_pair.o $C/conp_neigh.o $C/conp_ghost.o $C/conp_reneigh.o \
  $C/conp_fix.o $C/conp_dev.o $C/conp_pairstyle.o $C/conp_ghostmap.o $C/conp_ewaldquery.o $C/conp_host.o
