#!/bin/bash
# On the GPU box, end of round 2: rocprofv3 --kernel-trace --stats of the default bench.py (DDPG headline + the sac / naf /
# kl sub-records), the KL throughput script and the latency-mode script.  Outputs under gpurun_out/r02b_prof/.
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=$PWD/gpurun_out/r02b_prof
rm -rf $OUT && mkdir -p $OUT
rocprofv3 --kernel-trace --stats -d $OUT/stats -o stats -- python3 bench.py --full --no-cpu-baseline > $OUT/bench_under_rocprof.json 2> $OUT/stats.err || exit 1
python scripts/rocpd_extract.py --db $(find $OUT/stats -name "*_results.db" | head -1) --stats --out $OUT/r02b_bench_default || exit 1
python bench.py --full > $OUT/bench_plain.json 2> $OUT/bench_plain.err || exit 1
python scripts/bench_kl.py --tag r02 --cpu_updates 100 > $OUT/kl_bench.log 2>&1 || exit 1
tail -5 $OUT/kl_bench.log
python -c "
import json
d = json.loads(open('$OUT/bench_plain.json').read().strip().splitlines()[-1])
print('ddpg', d['value'], d['roofline']['frac'], '| sac', d['sac']['value'], d['sac']['roofline']['frac'], '| naf', d['naf']['value'], d['naf']['roofline']['frac'], '| kl', d['kl']['value'], d['kl']['roofline']['frac'], d['kl']['kernel'])
print('cpu', d['cpu_baseline'])
"
