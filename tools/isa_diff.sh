#!/bin/bash
# Are the device kernels of two builds of the library the same instructions?
#   tools/isa_diff.sh <objdir A> <objdir B> [object names ...]        (default: the seven vv_raymarch* objects)
# Takes the gfx950 code object out of each object file's fat binary, disassembles it and compares the text with addresses and
# encodings stripped (branch targets are printed as symbol + offset, so a moved function does not show).  Needs no GPU.
# Used for: shared helpers moved from vv_raymarch.hip into vv_layout.h (profiles/EXPERIMENTS.md).
set -e -o pipefail
A=$1; B=$2; shift 2
NAMES=${*:-vv_raymarch vv_raymarch_big vv_raymarch_brick vv_raymarch_brick_cached vv_raymarch_zpair vv_raymarch_zfast vv_raymarch_xpair}
LLVM=${LLVM:-/opt/rocm/llvm/bin}
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
rc=0
for n in $NAMES; do
    for side in A B; do
        dir=$A; [ $side = B ] && dir=$B
        $LLVM/llvm-objcopy --dump-section .hip_fatbin=$T/$side.fb $dir/$n.o
        $LLVM/clang-offload-bundler --unbundle --type=o --input=$T/$side.fb --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/$side.co
        $LLVM/llvm-objdump -d --no-show-raw-insn $T/$side.co | sed -E 's/^ *[0-9a-f]+://; s/[[:space:]]*\/\/ [0-9A-Fa-f]+:.*$//; s/^[0-9a-f]+ </</' | grep -v 'file format' > $T/$side.s
    done
    kernels=$(grep -c -E '^<.*(rad_kernel|march_kernel|march_phong_kernel).*>:$' $T/B.s || true)
    if cmp -s $T/A.s $T/B.s; then verdict="identical"; else verdict="DIFFERENT"; rc=1; fi
    echo "$n: $kernels kernels, $(wc -l < $T/B.s) lines of disassembly: $verdict (code object bytes: $(cmp -s $T/A.co $T/B.co && echo identical || echo differ))"
done
exit $rc
