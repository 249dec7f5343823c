# on the GPU box: tests, default bench, rocprofv3 kernel stats and PMC traffic of the same command
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bash scripts/final_profile.sh OUTDIR}
mkdir -p $OUT
timeout 600 python -m pytest tests -m gpu -q -x -o faulthandler_timeout=240 > $OUT/tests.log 2>&1; tail -3 $OUT/tests.log
timeout 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; python -c "
import json; d=json.load(open('$OUT/bench.json')); print('bench', round(d['value']), d['ms_per_step'], d['roofline']['frac'], d['cpu_baseline']['value'], d['cpu_baseline']['cores'], d.get('dense_reference',{}).get('value'))"
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ktrace -o k -- python3 bench.py --no-cpu-baseline --full > $OUT/bench_prof.json 2>/dev/null
ls $OUT/ktrace/* | head
bash scripts/pmc_passes.sh final > $OUT/pmc.log 2>&1; tail -30 $OUT/pmc.log | grep -E "^==|HBM"
