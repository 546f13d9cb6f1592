#!/bin/bash
# Compares the gfx950 device code objects of kernel sources between a git revision and the working tree:
#   tools/compare_codeobj.sh [--symbols] BASE_REV conv_bx3 conv_sp ...        (names of starcop_amd/csrc/*.hip, without the suffix)
# Both trees are built one after the other in the SAME scratch directory with the Makefile's own rules plus --save-temps=obj (the
# compilation-unit id that hipcc puts into every code object is a hash of the paths on its command line), then the
# <file>-hip-amdgcn-amd-amdhsa-gfx950.out files are compared byte for byte.  The .out and .s files of both sides stay under
# $WORK/base and $WORK/new for a closer look (diff the .s for the instructions and the .vgpr_count / .sgpr_count / LDS metadata).
# --symbols: compare kernel by kernel instead (tools/codeobj_symbols.py on the two .s files): for a change that removes instantiations,
# so that whole files differ, every kernel left must still read "identical", and the register / LDS / scratch figures of both sides are listed.
set -eu
symbols=0
if [ "$1" = --symbols ]; then symbols=1; shift; fi
base=$1; shift
root=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
WORK=${WORK:-${TMPDIR:-/tmp}/sc_codeobj}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$WORK"

build() {      # $1 = base | new; the tree is in $WORK/tree
  local objs=() f
  for f in "${FILES[@]}"; do objs+=("$f.o"); done
  make -C "$WORK/tree/starcop_amd/csrc" -j"${JOBS:-8}" HIPCC="$HIPCC --save-temps=obj" "${objs[@]}" > "$WORK/$1.log" 2>&1
  mkdir -p "$WORK/$1"
  for f in "${FILES[@]}"; do
    mv "$WORK/tree/starcop_amd/csrc/$f-hip-amdgcn-amd-amdhsa-gfx950.out" "$WORK/tree/starcop_amd/csrc/$f-hip-amdgcn-amd-amdhsa-gfx950.s" "$WORK/$1/"
  done
  rm -rf "$WORK/tree"
}
FILES=("$@")

rm -rf "$WORK/tree" "$WORK/base" "$WORK/new"
mkdir -p "$WORK/tree"
git -C "$root" archive "$base" starcop_amd/csrc include | tar -x -C "$WORK/tree"
build base
mkdir -p "$WORK/tree/starcop_amd"
cp -r "$root/include" "$WORK/tree/include"
cp -r "$root/starcop_amd/csrc" "$WORK/tree/starcop_amd/csrc"
make -C "$WORK/tree/starcop_amd/csrc" clean > /dev/null
build new

rc=0
for f in "${FILES[@]}"; do
  if [ $symbols = 1 ]; then
    echo "== $f"
    python3 "$root/tools/codeobj_symbols.py" "$WORK/base/$f-hip-amdgcn-amd-amdhsa-gfx950.s" "$WORK/new/$f-hip-amdgcn-amd-amdhsa-gfx950.s" || rc=1
    continue
  fi
  if cmp -s "$WORK/base/$f-hip-amdgcn-amd-amdhsa-gfx950.out" "$WORK/new/$f-hip-amdgcn-amd-amdhsa-gfx950.out"; then echo "$f: identical"
  else echo "$f: DIFFERS"; rc=1; fi
done
exit $rc
