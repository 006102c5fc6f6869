#!/bin/bash
# tools/build_variant.sh <name> <extra hipcc flags...>  ->  build/libfovpt_<name>.so, for FOVPT_SO=
# A second build of the library with extra compiler flags (a -DFOVPT_... knob for an A/B, or the diagnostic build
# -DFOVPT_V_STEPSTAT=1 that tools/stepstat.py, stepcount.py, raystat.py and raytrace_dump.py need).  It drives csrc/Makefile
# (EXTRA is appended to its FLAGS) in a temporary copy of csrc/, so the product's objects and libfovpt.so are not touched.
# A diagnostic build of k_traverse may fall below the product's eight waves per SIMD: the build guard lets that pass here
# (--allow-low-occupancy); scratch use in a per-frame kernel still fails the build.
set -euo pipefail
[ $# -ge 1 ] || { echo "usage: $0 <name> [extra hipcc flags...]" >&2; exit 2; }
NAME=$1; shift
ROOT=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
PKG=fovpathtracing_optixcodelatest_amd
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
# the same relative layout as the tree: csrc/ includes ../../include
mkdir -p "$TMP/$PKG" "$ROOT/build"
cp -r "$ROOT/include" "$TMP/include"
cp -r "$ROOT/$PKG/csrc" "$TMP/$PKG/csrc"
make -C "$TMP/$PKG/csrc" -s clean
rm -f "$TMP/$PKG/csrc"/*.res
make -C "$TMP/$PKG/csrc" -s -j"${MAX_JOBS:-8}" EXTRA="$*" CHECK_FLAGS=--allow-low-occupancy libfovpt.so
cp "$TMP/$PKG/csrc/libfovpt.so" "$ROOT/build/libfovpt_$NAME.so"
echo "$ROOT/build/libfovpt_$NAME.so"
