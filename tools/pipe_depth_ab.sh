# fgreg.pipeline depth A/B (run on the GPU box from the repo root): bench lines per workload
# at fgreg.pipeline.DEPTH 1 / 2 / 3, same box, summary to stdout
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
for wl in modelnet 3dmatch 3dlomatch; do for dp in 1 2 3; do
  f=$OUT/bench_${wl}_pd$dp
  timeout -k 10 300 python -c "
import runpy, sys
sys.path.insert(0, 'boosting-fine-grained-feature-fusion-in-3d-point-cloud-registration_amd')
import fgreg.pipeline
fgreg.pipeline.DEPTH = $dp
sys.argv = ['bench.py'] + sys.argv[1:]
runpy.run_path('bench.py', run_name='__main__')" --workload $wl --steps 50 --warmup 10 --no-cpu-baseline > $f.json 2> $f.err || { tail -20 $f.err; exit 1; }
  python3 -c "
import json; d=json.loads(open('$f.json').read().strip().splitlines()[-1]); print('$wl depth $dp', round(d['value'],1), 'pairs/s', round(d['ms_per_step'],3), 'ms/step')"
done; done
