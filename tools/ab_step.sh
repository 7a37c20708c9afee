#!/bin/bash
# In-situ A/B of one tuning knob: runs bench.py (train step, or the sampler for sample_split) once per value, twice interleaved, and
# prints ms per step -- the way every "measured" entry of DESIGN.md section 8 was taken (same box, same call).
#   usage (GPU box): bash tools/ab_step.sh <knob>        e.g.  bash tools/ab_step.sh gemm5
#   knobs: sumsq_fold  VBX_SUMSQ_FOLD      1 0    clip norm from the slab-reduce partials
#          factors     VBX_ADALN_FACTORS   1 0    adaLN weight gradients in factor form vs materialised
#          sample_split VBX_SAMPLE_SPLIT   2 1    sampler: two concurrent half batches vs one stream
#          gemm5       VBX_GEMM5           1 0    weight-stationary to_qkv / FeedForward-in (train step)
#          gemm5_sample VBX_GEMM5          1 0    the same in the 64-interval sampler
#          wgrad_overlap VBX_WGRAD_OVERLAP 1 0    weight gradients on the side stream vs in line (the stage columns are the in-line
#                                                 launches either way: the stage table is taken with the overlap off, include/vbx.h)
cd ${GRAFT_REPO_ROOT:-$(dirname $0)/..}
case "$1" in
  sumsq_fold) V=VBX_SUMSQ_FOLD; S="1 0";; factors) V=VBX_ADALN_FACTORS; S="1 0";;
  sample_split) V=VBX_SAMPLE_SPLIT; S="2 1";;
  gemm5|gemm5_sample) V=VBX_GEMM5; S="1 0";;
  wgrad_overlap) V=VBX_WGRAD_OVERLAP; S="1 0";;
  *) sed -n 2,11p $0; exit 1;;
esac
ARGS="--full --steps 30 --warmup 8 --no-cpu-baseline --no-sample"
[ "$1" = gemm5_sample ] && ARGS="--full --mode sample --steps 3 --warmup 1 --no-cpu-baseline"
[ "$1" = sample_split ] && ARGS="--full --mode sample --steps 3 --warmup 1 --no-cpu-baseline"
for i in 1 2; do for s in $S; do
  env $V=$s timeout 300 python bench.py $ARGS 2>/dev/null | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read()); k = {x['stage']: x['us_per_launch'] for x in d.get('roofline', {}).get('kernels', [])}
print('$V=$s', d['ms_per_step'], 'ms;', 'bwd attention', k.get('bwd attention'), 'wgrad', k.get('wgrad (4 GEMMs)'), 'to_qkv', k.get('fwd to_qkv'), 'ff_in', k.get('fwd ff_in'))"
done; done
