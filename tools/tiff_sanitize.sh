#!/bin/bash
# The TIFF reader under AddressSanitizer + UBSan as a stand-alone host program (never loaded into Python, never on the
# GPU): builds tests/tiff_san_main.cpp with the reader's translation unit, writes every valid test file and its
# corruption sweep (tests/tiff_files.py) into a scratch directory and runs the program over it.
# Exit status 0 and no sanitizer report is the criterion.   usage: tools/tiff_sanitize.sh [scratch directory]
set -euo pipefail
cd "$(dirname "$0")/.."
WORK=${1:-$(mktemp -d)}
mkdir -p "$WORK/files"
g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
    diffsplitting_amd/csrc/dsx_tiff.cpp tests/tiff_san_main.cpp -o "$WORK/tiff_san"
echo "files written: $(python tests/tiff_files.py "$WORK/files")"
"$WORK/tiff_san" "$WORK/files"
