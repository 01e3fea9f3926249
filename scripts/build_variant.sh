#!/bin/bash
# Build an experimental variant of libenf_hip.so:  scripts/build_variant.sh NAME "-DFLAG=.. -f.." ["src1 src2 .."]
# -> variants/libenf_NAME.so (git-ignored, travels to the GPU box); select with ENF_HIP_LIB=variants/libenf_NAME.so
# With a third argument only those sources are compiled with the flags; the rest are the in-tree objects (run `make` first).
set -e
cd "$(dirname "$0")/.."
NAME=$1; FLAGS=$2; ONLY=$3
mkdir -p variants build_variants/$NAME
SRC=enf-pde_amd/csrc
# the Makefile's sources (the whole C-ABI) plus enf_debug
ALL="$(sed -n 's/^SRCS *= *//p' $SRC/Makefile) enf_debug"
[ "$ALL" != " enf_debug" ] || { echo "no SRCS line in $SRC/Makefile" >&2; exit 1; }
OBJS=""
for f in $ALL; do
  if [ -z "$ONLY" ] || [[ " $ONLY " == *" $f "* ]] || [ ! -f $SRC/$f.o ]; then
    ( /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unknown-pragmas $FLAGS -c $SRC/$f.hip -o build_variants/$NAME/$f.o ) &
    OBJS="$OBJS build_variants/$NAME/$f.o"
  else
    OBJS="$OBJS $SRC/$f.o"
  fi
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS -o variants/libenf_$NAME.so
echo built variants/libenf_$NAME.so
