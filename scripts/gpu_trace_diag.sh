#!/bin/bash
# recurrence phase traces (KCTC_REC_TRACE) under diagnostic settings: TRACES="tag:ENV=V,ENV2=V ..."
set -o pipefail
export OUT=${OUT:-bench_out}  # where the logs and results go
mkdir -p $OUT
for spec in $TRACES; do
  tag=${spec%%:*}; envs=${spec#*:}
  mkdir -p $OUT/tr_$tag
  env ${envs//,/ } KCTC_REC_TRACE=$OUT/tr_$tag timeout -k 10 200 python bench.py --config ${CFG:-1} --steps 1 --warmup 0 --no-cpu-baseline --no-profile --no-loss-match --no-h2d-pass > $OUT/tr_$tag.log 2>&1 || { echo TRACE_FAILED $tag; tail -3 $OUT/tr_$tag.log; exit 1; }
  echo "== $tag"; python scripts/trace_rec.py $OUT/tr_$tag/rec_fwd.bin $OUT/tr_$tag/rec_bwd.bin | grep -v "shader clock" | tee $OUT/tr_$tag.txt
  rm -f $OUT/tr_$tag/*.bin  # (the stamps are tens of MB; the summary stays)
done
