#!/bin/sh
# usage: tools/kernel_regs.sh [pattern] [extra -D flags]  -> register / scratch / static LDS usage of the kernels in encode_fused.hip
# (SRC=train tools/kernel_regs.sh opt_rows: another file of csrc/)
cd "$(dirname "$0")/.."
PAT="${1:-gemm_kernel}"; [ $# -gt 0 ] && shift
SRC="${SRC:-encode_fused}"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -Wno-unused-function -Wno-inline-asm \
  -Rpass-analysis=kernel-resource-usage "$@" -c "multimodal-sae_amd/csrc/$SRC.hip" -o /tmp/ef_$$.o 2>/tmp/ef_$$.err
grep "remark:" /tmp/ef_$$.err | grep -A9 "$PAT" | grep -E "Function Name| VGPRs:|TotalSGPRs|ScratchSize|Occupancy|VGPRs Spill|LDS Size" | \
  sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - - - - | sed 's/Function Name: //' | cut -c1-230
rm -f /tmp/ef_$$.o /tmp/ef_$$.err
