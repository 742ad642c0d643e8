#!/bin/bash
# Builds libdsx.so for gfx950 in-tree (cross-compiles without a GPU).  DSX_EXTRA_FLAGS adds compiler flags; DSX_OBJ and
# DSX_OUT (relative to this directory) redirect the objects and the library: tools/build_variant.sh.
set -e
cd "$(dirname "$0")"
OUT=${DSX_OUT:-../libdsx.so}
OBJ=${DSX_OBJ:-_obj}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $DSX_EXTRA_FLAGS"
mkdir -p $OBJ
# every source of the library: kernels (*.hip) and host translation units (*.cpp, compiled as HIP too)
SRCS="dsx_conv.hip dsx_ops.hip dsx_attn.hip dsx_lpips.hip dsx_resize.hip dsx_eval.hip dsx_steps.hip dsx_validate.hip dsx_select.hip dsx_model.cpp dsx_plan.cpp dsx_exec.cpp dsx_tiles.cpp dsx_lpips.cpp dsx_resize.cpp dsx_select.cpp dsx_tiff.cpp"
# a changed flag set rebuilds everything
if [ "$(cat $OBJ/.flags 2>/dev/null)" != "$FLAGS" ]; then rm -f $OBJ/*.o; echo "$FLAGS" > $OBJ/.flags; fi
stale() {   # stale OBJECT FILE...: the object is missing or older than one of the files
  local o=$1; shift
  [ -f $o ] || return 0
  for d in "$@"; do [ $d -nt $o ] && return 0; done
  return 1
}
pids=()
OBJS=""
for f in $SRCS; do
  case $f in
    *.hip) deps="dsx_kernels.h dsx_reduce.h $(echo *.inc)"; lang="" ;;     # included bodies (dsx_conv_ws_item.inc)
    *) deps="dsx_rt.h dsx_kernels.h ../../include/dsx.h"; lang="-x hip" ;;
  esac
  OBJS="$OBJS $OBJ/$f.o"
  if stale $OBJ/$f.o $f $deps; then
    rm -f $OBJ/$f.o                       # a failed compile must not leave a stale object to link
    hipcc $FLAGS $lang -c $f -o $OBJ/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p || { echo "build.sh: a compile failed" >&2; exit 1; }; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $OBJS
echo "built $(realpath $OUT)"
