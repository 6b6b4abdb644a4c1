#!/bin/bash
# Build libhdisort.so with extra compile flags (the kernels' compile-time knobs:
# -DHD_LAYER_PREFETCH=0, -DHD_NT_MIN_SOLVES=..., -DHD_RAD_USER_WAVES=2, ...) into
# ab_libs/libhdisort_NAME.so, for A/B runs against the in-tree library on one box
# (HD_LIB_PATH=ab_libs/libhdisort_NAME.so python ...):
#   bash scripts/ab/build_variant.sh NAME -DFLAG=VALUE ...
set -e
NAME=$1; shift
OUT=ab_libs/obj_$NAME; mkdir -p $OUT
C=pyharp_amd/csrc
for src in hd_kernels.hip hd_team_mfma.hip hd_rad.hip hd_harp.hip hd_api.cpp hd_ncread.cpp hd_rad_wide.hip hd_beer.hip; do
  extra=""; [ $src = hd_team_mfma.hip -o $src = hd_beer.hip ] && extra="-mllvm -disable-machine-licm"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip "$@" $extra -c $C/$src -o $OUT/$src.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ab_libs/libhdisort_$NAME.so $OUT/*.o -lz
rm -rf $OUT
echo ab_libs/libhdisort_$NAME.so
