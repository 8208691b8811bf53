#!/bin/bash
# Builds variants/lib_<name>.so = the product library with extra compiler flags and / or a source patch (A/B experiments, the
# stamp build), in a scratch copy of csrc/ so the in-tree build is untouched.
# Usage: bash tools/build_variant.sh <name> "<extra flags>" [patch against simgan_amd/csrc, e.g. tools/diag/step4_stamps.patch]
# With a patch the test library is built too (variants/lib_<name>_test.so): a patch's hooks live there.
# On the GPU box: run the tool on a copy of the tree with these in place of simgan_amd/libsimgan_hip{,_test}.so.
set -eu
name=$1; extra=${2:-}; patch=${3:-}
root=$(cd "$(dirname "$0")/.." && pwd)
work=/tmp/sg_variant_$name
rm -rf $work && mkdir -p $work/simgan_amd $root/variants
cp -r $root/simgan_amd/csrc $work/simgan_amd/ && cp -r $root/include $work/ && rm -rf $work/simgan_amd/csrc/build
targets=../libsimgan_hip.so
if [ -n "$patch" ]; then
    patch=$(realpath "$patch")
    (cd $work && git apply "$patch")
    targets="$targets ../libsimgan_hip_test.so"
fi
make -s -C $work/simgan_amd/csrc -j8 $targets CXXFLAGS="-O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-result -mllvm -amdgpu-kernarg-preload-count=16 $extra" 2>&1 | grep -E "error|warning" || true
cp $work/simgan_amd/libsimgan_hip.so $root/variants/lib_$name.so
[ -z "$patch" ] || cp $work/simgan_amd/libsimgan_hip_test.so $root/variants/lib_${name}_test.so
ls -la $root/variants/lib_$name*.so
