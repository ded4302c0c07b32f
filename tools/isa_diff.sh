#!/bin/bash
# Are the device kernels of two builds of the library the same instructions?
#   tools/isa_diff.sh <objdir A> <objdir B> [object names ...]        (default: the seven vv_raymarch* objects)
# Takes the gfx950 code object out of each object file's fat binary, disassembles it and compares the text with addresses and
# encodings stripped (branch targets are printed as symbol + offset, so a moved function does not show).  Needs no GPU.
# SKIP=<regex>: functions whose (mangled) symbol matches are left out on both sides, e.g. SKIP=fill for the fill kernels; what remains -- its
# function labels included, so the lists of the remaining kernels too -- is compared.  The literal of a pc-relative call sequence (s_getpc_b64, s_add_u32)
# and the alignment padding behind a function depend on where the neighbouring functions lie, not on the function: both are masked.
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
        $LLVM/llvm-objdump -d --no-show-raw-insn $T/$side.co | sed -E 's/^ *[0-9a-f]+://; s/[[:space:]]*\/\/ [0-9A-Fa-f]+:.*$//; s/^[0-9a-f]+ </</' | grep -v 'file format' |
            awk -v skip="$SKIP" '
                /^<.*>:$/ { drop = skip != "" && $0 ~ skip; held = "" }
                drop { next }
                pcrel && /s_add_u32/ { sub(/0x[0-9a-f]+$/, "<pc-relative>") }                 # the distance to a called function, which moves with its neighbours
                { pcrel = /s_getpc_b64/ }
                /^[[:space:]]*s_nop 0$/ { held = held $0 "\n"; next }                          # alignment padding behind a function: s_nop 0 up to "...", an empty line or the next label
                /^[[:space:]]*(\.\.\.)?$/ { held = ""; next }
                { printf "%s", held; held = ""; print }' > $T/$side.s
    done
    kernels=$(grep -c -E '^<.*_kernel.*>:$' $T/B.s || true)
    if cmp -s $T/A.s $T/B.s; then verdict="identical"; else verdict="DIFFERENT"; rc=1; fi
    echo "$n: $kernels kernels, $(wc -l < $T/B.s) lines of disassembly${SKIP:+ without /$SKIP/}: $verdict (code object bytes: $(cmp -s $T/A.co $T/B.co && echo identical || echo differ))"
done
exit $rc
