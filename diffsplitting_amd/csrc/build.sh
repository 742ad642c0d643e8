#!/bin/bash
# Builds libdsx.so for gfx950 in-tree (cross-compiles without a GPU).  DSX_EXTRA_FLAGS adds compiler flags; DSX_OBJ and
# DSX_OUT (relative to this directory) redirect the objects and the library: tools/build_variant.sh.
set -e
cd "$(dirname "$0")"
OUT=${DSX_OUT:-../libdsx.so}
OBJ=${DSX_OBJ:-_obj}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $DSX_EXTRA_FLAGS"
mkdir -p $OBJ
# every source of the library: kernels (*.hip) and host translation units (*.cpp, compiled as HIP too); the longest
# compile first
SRCS="dsx_conv_mfma.hip dsx_conv_ws.hip dsx_conv_img.hip dsx_conv_direct.hip dsx_conv.hip dsx_ops.hip dsx_attn.hip dsx_lpips.hip dsx_resize.hip dsx_tiles.hip dsx_eval.hip dsx_msssim.hip dsx_steps.hip dsx_validate.hip dsx_select.hip dsx_refine.hip dsx_calib.hip dsx_quantiles.hip dsx_consistency.hip dsx_model.cpp dsx_plan.cpp dsx_exec.cpp dsx_tiles.cpp dsx_eval.cpp dsx_lpips.cpp dsx_resize.cpp dsx_select.cpp dsx_refine.cpp dsx_calib.cpp dsx_quantiles.cpp dsx_consistency.cpp dsx_tiff.cpp"
# a changed flag set rebuilds everything
if [ "$(cat $OBJ/.flags 2>/dev/null)" != "$FLAGS" ]; then rm -f $OBJ/*.o; echo "$FLAGS" > $OBJ/.flags; fi
stale() {   # stale OBJECT FILE...: the object is missing or older than one of the files
  local o=$1; shift
  [ -f $o ] || return 0
  for d in "$@"; do [ $d -nt $o ] && return 0; done
  return 1
}
JOBS=${MAX_JOBS:-16}   # compiles in flight
running=0
failed=0
OBJS=""
for f in $SRCS; do
  case $f in
    *.hip) deps="$(echo *.h *.inc)"; lang="" ;;     # every header and included body (dsx_conv_ws_item.inc) of this directory
    *) deps="dsx_rt.h dsx_kernels.h ../../include/dsx.h"; lang="-x hip" ;;
  esac
  OBJS="$OBJS $OBJ/$f.o"
  if stale $OBJ/$f.o $f $deps; then
    rm -f $OBJ/$f.o                       # a failed compile must not leave a stale object to link
    if [ $running -ge $JOBS ]; then wait -n || failed=1; running=$((running - 1)); fi
    hipcc $FLAGS $lang -c $f -o $OBJ/$f.o &
    running=$((running + 1))
  fi
done
while [ $running -gt 0 ]; do wait -n || failed=1; running=$((running - 1)); done
for o in $OBJS; do [ -f $o ] || failed=1; done
if [ $failed -ne 0 ]; then echo "build.sh: a compile failed" >&2; exit 1; fi
# (--no-undefined: the conv table names kernels that another object defines; one that none defines must fail here, not at load)
hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined -o $OUT $OBJS
echo "built $(realpath $OUT)"
