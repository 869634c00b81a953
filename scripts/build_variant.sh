#!/bin/bash
# Build a variant of the engine under build/variants/NAME.so with extra compiler flags (e.g. -DZGPU_WALK_STATS).
# Usage: scripts/build_variant.sh NAME FLAGS...   -- select it with ZAMD_GPU_LIB=$PWD/build/variants/NAME.so
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/build/variants; OBJ=$ROOT/build/variants/obj_$NAME
mkdir -p $OBJ
for f in $(cd $ROOT/zlib_amd/csrc && ls *.hip | sed s/.hip$//); do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wno-unused-value -Wno-unused-result "$@" -c $ROOT/zlib_amd/csrc/$f.hip -o $OBJ/$f.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/$NAME.so $OBJ/*.o -ldl
rm -rf $OBJ
echo built $OUT/$NAME.so
