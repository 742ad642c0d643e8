#!/bin/bash
# usage: tools/build_variant.sh NAME "-DFLAG ..."  -> diffsplitting_amd/csrc/_variants/libdsx_NAME.so
# (diagnostic builds for timing experiments: select with DSX_LIB_PATH; the .so travels to the GPU box)
# The sources, flags and compile steps are those of csrc/build.sh, with objects and output of the variant's own.
set -e
CSRC="$(dirname "$0")/../diffsplitting_amd/csrc"
NAME=$1; EXTRA=$2
mkdir -p "$CSRC/_variants"
DSX_EXTRA_FLAGS="$EXTRA" DSX_OBJ=_obj_$NAME DSX_OUT=_variants/libdsx_$NAME.so "$CSRC/build.sh"
rm -rf "$CSRC/_obj_$NAME"
