#!/bin/bash
# Build an A/B variant of the library BESIDE the product one (in the build container; the .so travels with the snapshot):
#   tools/build_variant.sh tools/variants/stages3.so HN_WGRAD_STAGES=3 HN_WGRAD_MAXSLOT=6
# optionally from another source file:  SRC_MLP=path/to/hn_mlp_variant.hip tools/build_variant.sh out.so
# tools/ab.sh "label: LIB=tools/variants/stages3.so" then runs it through HN_LIB_PATH.
# The sources are the product build's (_lib.SOURCES); SRC_MLP / SRC_RENDER replace their entry.  Flags as _lib.build().
out=$1; shift
cd "$(dirname "$0")/.."
mkdir -p "$(dirname "$out")"
csrc=hypernerf-torch_amd/csrc
defs=""; for kv in "$@"; do defs="$defs -D$kv"; done
names=$(python3 -c "from hypernerf_torch_amd import _lib; print(*_lib.SOURCES)") || exit 1
srcs=""
for s in $names; do
  case $s in
    hn_mlp.hip) srcs="$srcs ${SRC_MLP:-$csrc/$s}" ;;
    hn_render.hip) srcs="$srcs ${SRC_RENDER:-$csrc/$s}" ;;
    *) srcs="$srcs $csrc/$s" ;;
  esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -munsafe-fp-atomics -fPIC -shared $defs \
  -I$csrc -o "$out" $srcs && echo "built $out ($*)"
