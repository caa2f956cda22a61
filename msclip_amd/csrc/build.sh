#!/bin/bash
# Build libmsclip_hip.so in-tree for gfx950 (cross-compiles without a GPU).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffast-math -fno-finite-math-only -Wall -Wno-unused-function"
mkdir -p build
objs=()
pids=()
for f in gemm gemm_small gemm_skinny attention qkv_attention attention_bwd backward backward_conv rows conv front loss pack api plan comm optim clip ema probe input color metrics; do
  stale=0
  for d in $f.hip common.h gemm_epilogue.h plan.h multi_tensor.h ../../include/msclip_hip.h ../../include/msclip_ext.h ../../include/msclip_ext2.h ../../include/msclip_ext3.h ../../include/msclip_ext4.h ../../include/msclip_ext5.h ../../include/msclip_input.h ../../include/msclip_color.h ../../include/msclip_metrics.h; do
    if [ ! -f build/$f.o ] || [ $d -nt build/$f.o ]; then stale=1; fi
  done
  if [ $f = input ] && [ input_body.h -nt build/$f.o ]; then stale=1; fi      # (only input.hip includes it)
  if [ $f = color ] && [ color_body.h -nt build/$f.o ]; then stale=1; fi      # (only color.hip includes it)
  if [ $f = metrics ] && [ rank_body.h -nt build/$f.o ]; then stale=1; fi     # (only metrics.hip includes it)
  if [ $stale = 1 ]; then
    # no fast-math for pack.hip (tensor algebra that must come out bitwise: IEEE division / square root, no contraction) and clip.hip
    # (NaN / Inf must travel), which is why clip.hip is not part of optim.hip: AdamW's division and sqrtf ARE compiled with fast-math,
    # and moving either across that line changes bits; ema.hip (the EMA's multiply, multiply, add must stay three roundings: no fma);
    # probe.hip (the hi/lo split's x - float(hi) and the accurate expf / logf of the classifier's row pass); input.hip (floor(x + 0.5),
    # the weights' division by their sum and the unfused multiply-adds of the resampling: input_body.h must give the host's bits); color.hip (the blend's two roundings, the
    # IEEE divisions of the HSV conversions and the blur's unfused multiply-adds: color_body.h must give the host's bits); metrics.hip
    # (the rank counts' comparisons must see NaN, +-0 and denormals as IEEE does: rank_body.h must give the host's counts)
    if [ $f = pack ] || [ $f = clip ] || [ $f = ema ] || [ $f = probe ] || [ $f = input ] || [ $f = color ] || [ $f = metrics ]; then FL="${FLAGS/-ffast-math -fno-finite-math-only/-fno-fast-math -ffp-contract=off}"; else FL="$FLAGS"; fi
    $HIPCC $FL -c $f.hip -o build/$f.o &
    pids+=($!)
  fi
  objs+=(build/$f.o)
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o libmsclip_hip.so "${objs[@]}"
echo "built $(pwd)/libmsclip_hip.so"
