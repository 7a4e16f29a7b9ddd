#!/bin/bash
# Build a scratch variant of the HIP library with extra compiler flags for same-box A/B runs:
#   bash tools/build_variant.sh prio -DMMDIT_STATIC_PRIO     ->  tools/scratch/prio/libmmdit_hip.so   (select with MMDIT_LIB=...)
# Sources and per-source flags are build.py's SOURCES / SOURCE_FLAGS, so a variant is a complete library.
# The scratch directory is git-ignored but travels to the GPU box with gpurun.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
out=tools/scratch/$name
mkdir -p $out
list=$(python3 -c 'import sys; sys.path.insert(0, "stable-diffusion-3-from-scratch_amd"); import build as b; [print(s, *b.SOURCE_FLAGS.get(s, [])) for s in b.SOURCES]')
while read -r src flags; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $flags "$@" -c stable-diffusion-3-from-scratch_amd/csrc/$src -o $out/${src%.hip}.o 2>/dev/null &
done <<< "$list"
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libmmdit_hip.so $out/*.o
rm -f $out/*.o
ls -la $out/libmmdit_hip.so
