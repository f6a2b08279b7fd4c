#!/bin/bash
# Builds a study variant of libeegfx.so (compile-time macros of the product sources) for library
# A/Bs (bench.py --lib, tools/epochs_bench.py --lib), through the product Makefile: its source
# list is the only one.
#   tools/build_ab_lib.sh <out_dir> "-DEEGFX_TRACK_X=0"
set -euo pipefail
OUT=${1:?out dir}; DEFS=${2:-}
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
make -C "$(dirname "$0")/../eeg_dataanalysispackage_amd/csrc" BUILD="$OUT/build" \
  LIB="$OUT/libeegfx.so" EXTRA_DEFS="$DEFS" -j16
rm -rf "$OUT/build"
