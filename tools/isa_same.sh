#!/bin/bash
# Check that the work tree's t2_kernels.hip compiles to the same gfx950 device code as a git revision's (for
# refactors; needs no GPU, about a minute):
# tools/isa_same.sh REV  ->  exit 0 if the assemblies are equal, else 1 and the names of the kernels that differ
set -e -o pipefail
cd "$(dirname "$0")/.."
rev=$1
C=gr-dvbt2ll_amd/csrc
mkdir -p exp_build/isa_rev
git show "$rev:$C/t2_kernels.hip" > exp_build/isa_rev/t2_kernels.hip
git show "$rev:$C/t2_kernels.h" > exp_build/isa_rev/t2_kernels.h
# device assembly of DIR/t2_kernels.hip without the per-compilation __hip_cuid_ symbol, each line prefixed with
# the function label it follows
asm() {
  /opt/rocm/bin/hipcc -std=c++17 -O3 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -I$1 --cuda-device-only -S $1/t2_kernels.hip -o - |
    grep -v __hip_cuid_ | awk '/^[_A-Za-z][^ \t]*:/ { k = $1 } { print k "\t" $0 }' > $2
}
asm exp_build/isa_rev exp_build/isa_rev.s & p=$!
asm $C exp_build/isa_tree.s
wait $p
n=$(grep -c '\.amdhsa_kernel ' exp_build/isa_tree.s)
if diff exp_build/isa_rev.s exp_build/isa_tree.s > exp_build/isa.diff; then
  echo "same device code as $rev: $n kernels, $(wc -l < exp_build/isa_tree.s) assembly lines"
else
  echo "device code differs from $rev ($(grep -c '^[<>]' exp_build/isa.diff) lines, exp_build/isa.diff) in:"
  sed -n 's/^[<>] \([^\t]*\):\t.*/\1/p' exp_build/isa.diff | sort -u | c++filt
  exit 1
fi
