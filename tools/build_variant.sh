#!/bin/bash
# usage: tools/build_variant.sh NAME file.hip [-DDEFS ...]  -> mapperatorinator_amd/lib/libmapperhip_NAME.so
# (only `file.hip` is recompiled with the defines; every other object comes from build/obj -- run `make` first)
set -e
cd "$(dirname "$0")/.."
name=$1; src=$2; shift 2
mkdir -p build/var_$name
base=$(basename $src .hip)
extra=; if [ $base = attention ]; then extra=-fno-slp-vectorize; fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -Wno-pass-failed -mllvm -amdgpu-kernarg-preload-count=14 $extra "$@" -c mapperatorinator_amd/csrc/$src -o build/var_$name/$base.o
# the other objects: one per unit of the Makefile's SRCS, the one list (never build/obj/*.o: an object left behind by a unit that has
# since been split or removed would define its symbols a second time)
objs=
for f in $(make -s print-srcs); do
  b=$(basename $f .hip)
  if [ $b = $base ]; then continue; fi
  if [ ! -f build/obj/$b.o ]; then echo "build/obj/$b.o is missing: run make first" >&2; exit 1; fi
  objs="$objs build/obj/$b.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs build/var_$name/$base.o -o mapperatorinator_amd/lib/libmapperhip_$name.so
echo built mapperatorinator_amd/lib/libmapperhip_$name.so
