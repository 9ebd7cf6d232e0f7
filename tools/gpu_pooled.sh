set -o pipefail
O=${OUT:-bench_out}; mkdir -p "$O"
timeout -k 10 300 python -u -m pytest tests/test_gpu_plane.py -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > $O/pyt_pooled.log 2>&1; r=$?; tail -3 $O/pyt_pooled.log; grep -E "FAILED|Error|assert" $O/pyt_pooled.log | head; [ $r = 0 ] || exit 1
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider > $O/pyt_pooledfull.log 2>&1; r=$?; tail -2 $O/pyt_pooledfull.log; grep -E "FAILED|Error" $O/pyt_pooledfull.log | head -5; [ $r = 0 ] || exit 1
mkdir -p $O/pooled
for w in hg19-dir1 hg19-nondir1 hg19-8s1c; do
  timeout -k 10 300 python bench.py --full --workload $w --steps 20 --warmup 3 --no-cpu-baseline > $O/pooled/$w.json 2> $O/pooled/$w.err || { tail -3 $O/pooled/$w.err; exit 1; }
  python -c "
import json; d=json.loads(open('$O/pooled/$w.json').read().strip().splitlines()[-1]); r=d['roofline']
print('$w', d['value'], d['ms_per_step'], 'k1a', r['kernel_ms'], 'iso', r['isolated_ms'])"
done
timeout -k 10 400 python bench.py --full --workload hg19mm9-32rep --steps 5 --warmup 1 --no-cpu-baseline > $O/pooled/rep.json 2> $O/pooled/rep.err || { tail -3 $O/pooled/rep.err; exit 1; }
python -c "
import json; d=json.loads(open('$O/pooled/rep.json').read().strip().splitlines()[-1]); r=d['roofline']
print('32rep', d['value'], d['ms_per_step'], 'k1a', r['kernel_ms'], 'iso', r['isolated_ms'], d['regions'])"
