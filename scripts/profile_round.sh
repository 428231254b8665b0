#!/bin/bash
# One gpurun call: headline bench line, rocprofv3 kernel trace + stats of the headline workload (one
# stream, so every ensemble dispatch is the priced 50k-row launch), then the PMC passes (scripts/pmc.sh).
# Outputs under $MOPO_OUT (default bench_out/); copy the ones to keep into profiles/<round>_*.
cd "${GRAFT_REPO_ROOT:-/root/repo}"
R=$PWD
OUT=${MOPO_OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 400 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail -5 $OUT/bench.err; exit 1; }
echo "bench ok"
cd /tmp && MOPO_ROLLOUT_SPLIT=1 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/prof" -o run -- \
  python "$R/bench.py" --full --no-cpu-baseline --no-c3 --no-alt-dtypes --train-epochs 0 > "$R/$OUT/prof_bench.json" 2> "$R/$OUT/prof.err" \
  || { tail -5 "$R/$OUT/prof.err"; exit 1; }
echo "rocprof ok"
cd "$R" && bash scripts/pmc.sh $OUT/pmc_summary.json
