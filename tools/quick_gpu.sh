#!/bin/bash
# usage (GPU box): tools/quick_gpu.sh <tag> [out-dir]  -> GPU tests + the short summary of the --full bench, logs under out-dir (default: out/)
R=$(cd "$(dirname "$0")/.." && pwd); tag=$1; OUT=${2:-$R/out}
mkdir -p $OUT
python3 -m pytest $R/tests -m gpu -x -q > $OUT/gpu_tests_$tag.log 2>&1; echo "tests rc=$? $(tail -1 $OUT/gpu_tests_$tag.log)"
python3 $R/bench.py --full --no-cpu-baseline --no-degeneracy 2> $OUT/bench_$tag.err | tail -1 > $OUT/bench_$tag.json
python3 -c "
import json
d=json.load(open('$OUT/bench_$tag.json'))
print(round(d['value']), 'kf/s', round(d['ms_per_step'],2), 'ms/step', {k: round(v,3) for k,v in d['stage_ms'].items()}, 'single', round(d['single_window']['ms_per_update'],3), round(d['single_window']['solve_ms'],4), 'sharded', round(d['time_sharded_window']['ms_per_lm_trial'],3), 'gm', round(d['graph_manager']['solve_ms_mean'],3), 'conv', round(d['with_convergence_exit']['value']))
"
