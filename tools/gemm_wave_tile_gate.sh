#!/bin/bash
# The gate of profiles/gemm_wave_tile.txt: the product's candidate GEMM without its element loop (tools/gemm_sweep.hip built with
# -DMSAE_ABL_NOEPI, 16x16x64 MFMAs, tile-major operands) against variants of the four-wave prototype (tools/gemm4w.hip), arms
# alternating, three runs each, power / sclk sampled beside each run (tools/smi_sample.sh).
#   tools/gemm_wave_tile_gate.sh build          compile both programs into tools/bin/ (no GPU needed)
#   tools/gemm_wave_tile_gate.sh run [7 11 ..]  prototype variants to alternate with the product (default 7); variant 8 (no staging)
#                                               brings the product's no-staging arm (SWEEP_CFG=8) with it.
#                                               Prints the sampler's line and the program's result line of every run.
# Every run has its own time limit, and nothing is started after a run that failed or whose outputs did not match.
set -o pipefail
cd "$(dirname "$0")/.."
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
if [ "$1" = build ]; then
  mkdir -p tools/bin
  "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-function tools/gemm4w.hip -o tools/bin/gemm4w &&
  "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Wno-unused-function -DMSAE_ABL_NOEPI tools/gemm_sweep.hip -o tools/bin/gemm_sweep_noepi
  exit $?
fi
shift
VARIANTS="${*:-7}"
REPS=${REPS:-800}
N=${GATE_N:-126976}
S=tools/smi_sample.sh
# the sampler prints its medians and the last lines of the program's output, the result line among them
ran() {  # name, the sampler's output
  echo "$2"
  echo "$2" | grep -q "best" || { echo "run $1 failed"; exit 4; }
}
prod() {  # name cfg
  out=$(SWEEP_D=2048 SWEEP_N=$N SWEEP_PACKED=1 SWEEP_SIGMA=32,32 SWEEP_CFG=$2 SWEEP_READY=1 bash $S $1 ready -- timeout -k 10 120 tools/bin/gemm_sweep_noepi $REPS 2>&1)
  ran $1 "$out"
}
proto() {  # name variant
  out=$(G4W_SIGMA=32 G4W_N=$N G4W_REPS=$REPS G4W_ONLY=$2 G4W_READY=1 bash $S $1 ready -- timeout -k 10 120 tools/bin/gemm4w 2>&1)
  ran $1 "$out"
  [ "$2" = 8 ] || echo "$out" | grep -q "checked: ok" || { echo "run $1: outputs do not match"; exit 3; }
}
for rep in 1 2 3; do
  [ "$VARIANTS" = 8 ] || prod product_r$rep 7
  for v in $VARIANTS; do
    if [ "$v" = 8 ]; then prod product_nostage_r$rep 8; fi
    proto proto${v}_r$rep $v
  done
done
