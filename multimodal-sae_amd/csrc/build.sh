#!/bin/sh
# Builds libmsae_hip.so, and its perturbed-schedule variant libmsae_hip_perturb.so, for gfx950 in-tree.
# -ffp-contract=off: every fused multiply-add in the kernels is an explicit fma/MFMA, so device
# arithmetic matches oracle/sae_oracle.c operation for operation.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../msae/_lib"
mkdir -p "$OUT"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -Wall -Wno-unused-function -Wno-inline-asm"
OBJS=""
for f in capi decode delta_decode recon refit nested_decode topk sparsify feature_stats coact act_hist pos_profile token_profile encode_f32 skip_gemm probe neighbors edit_topk batch_select jump_select encode_fused train; do
  "$HIPCC" $FLAGS -c "$HERE/$f.hip" -o "$OUT/$f.o" &
  OBJS="$OBJS $OUT/$f.o"
done
# The perturbed-schedule variant (tuning.h: MSAE_PERTURB, MSAE_GRID_CAP; tests/test_gpu_perturbed_schedule.py): only the
# translation units that read the two switches are compiled a second time, beside the product objects -- encode_fused (every
# instrumented header, the probes' counters and the variant-only exports: the ONE unit built with MSAE_PERTURB) and the two
# capped launchers of the exact fallback.  Every other object is linked as it is.
POBJS="$OBJS"
"$HIPCC" $FLAGS -DMSAE_PERTURB -DMSAE_PERTURB_MAX=256 -DMSAE_GRID_CAP=8 -c "$HERE/encode_fused.hip" -o "$OUT/encode_fused.perturb.o" &
for f in encode_f32 topk; do
  "$HIPCC" $FLAGS -DMSAE_GRID_CAP=8 -c "$HERE/$f.hip" -o "$OUT/$f.perturb.o" &
done
for f in encode_fused encode_f32 topk; do
  POBJS="$(echo "$POBJS" | sed "s| $OUT/$f\.o| $OUT/$f.perturb.o|")"
done
wait
"$HIPCC" --offload-arch=gfx950 -shared -fPIC $OBJS -o "$OUT/libmsae_hip.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC $POBJS -o "$OUT/libmsae_hip_perturb.so"
rm -f $OBJS $POBJS
echo "built $OUT/libmsae_hip.so $OUT/libmsae_hip_perturb.so"
