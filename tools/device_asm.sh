#!/bin/sh
# Device code of every translation unit of the kernel library, for comparing two trees kernel by kernel.
#   tools/device_asm.sh <csrc dir> <out dir>     then     diff -r <out dir of tree A> <out dir of tree B>
# Writes per source file NAME.s (gfx950 assembly, the Makefile's flags, device side only: no addresses, and the
# .amdhsa_* block of each kernel carries its registers, LDS and scratch) and NAME.res (the compiler's
# kernel-resource-usage remarks: VGPRs, AGPRs, SGPRs, spills, scratch, occupancy, LDS), with the source directory taken out
# of the remarks so that two trees compare equal when their code is.  Needs no GPU.  profiles/wave_ops_refactor.md used it.
set -eu
SRC=$(cd "$1" && pwd)
OUT=$2
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
cd "$SRC"
ls *.hip api.cpp | xargs -P "${JOBS:-8}" -I{} sh -c '
    n=${1%.*}
    '"$HIPCC"' -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math \
        -w -x hip --cuda-device-only -S "$1" -o "'"$OUT"'/$n.s" -Rpass-analysis=kernel-resource-usage 2>&1 |
        grep -E "remark:" | sed -E "s/^[^ ]*: remark: //" > "'"$OUT"'/$n.res"' _ {}
