#!/bin/bash
# Rebuilds the full source of a measured-and-rejected kernel variant from its patch under
# tools/probes/history/ (DESIGN.md §6 cites each one).  A patch's first line names its base: a
# product file at the commit where the variant was measured ("# base: <commit>:<path>", needs the
# git history, i.e. run it in the repository, not on the GPU box), or another history patch
# ("# base: patch:<name>.patch").
#   bash tools/probes/restore_variant.sh persistent_r02_pq2_fused [out.hip]
#   then build it like an ablation: hipcc ... -DFUSED_SRC='"<dir>/fused.hip"' window_probe.hip
# Without an output path the file is written to build/<name>/ under the base file's own name.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
restore() {  # restore <name> <out>
  local p="$HERE/history/$1.patch"
  local base
  base=$(head -1 "$p" | sed 's/^# base: //')
  local tmp
  tmp=$(mktemp)
  if [[ "$base" == patch:* ]]; then
    restore "$(basename "${base#patch:}" .patch)" "$tmp"
  else
    git -C "$HERE" show "$base" > "$tmp"
  fi
  tail -n +2 "$p" | patch -s -o "$2" "$tmp"
  rm -f "$tmp"
}
base_file() {  # base_file <name>: the product file at the bottom of the patch's chain
  local base
  base=$(head -1 "$HERE/history/$1.patch" | sed 's/^# base: //')
  if [[ "$base" == patch:* ]]; then base_file "$(basename "${base#patch:}" .patch)"
  else basename "${base#*:}"; fi
}
name=$1
out=${2:-$HERE/build/$name/$(base_file "$name")}
mkdir -p "$(dirname "$out")"
restore "$name" "$out"
echo "$out"
