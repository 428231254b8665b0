bash scripts/gpu.sh "tests:actor or full_pool or bf16x6 or mopo" || exit 1
OUT=${MOPO_OUT:-bench_out}
: > $OUT/actor_ab.txt
for i in 1 2; do
  for act in bf16x6 fp32; do
    timeout -k 10 150 python bench.py --full --no-cpu-baseline --no-c3 --no-alt-dtypes --train-epochs 0 --sac-steps 16 --actor-dtype $act > $OUT/aab.json 2>$OUT/aab.err || { tail -5 $OUT/aab.err; exit 1; }
    python -c "import json; d=json.loads(open('$OUT/aab.json').read().strip().splitlines()[-1]); k=d['kernel_ms_avg']; print('$act', round(d['value']/1e6,2), 'M/s ens', k['ensemble_fwd'], 'actor', k['actor'])" >> $OUT/actor_ab.txt
  done
done
cat $OUT/actor_ab.txt
