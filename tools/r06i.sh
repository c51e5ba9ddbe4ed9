# full GPU suite, smoke, the driver's bench command, FwFM-only and training step (tag $1)
T=${1:-r06i}
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
[ -n "$SKIP_TESTS" ] || { timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/${T}_t-all.log 2>&1 || { tail -30 $OUT/${T}_t-all.log; exit 1; }; tail -2 $OUT/${T}_t-all.log; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${T}_smoke.log 2>&1 || { tail -20 $OUT/${T}_smoke.log; exit 1; }
tail -2 $OUT/${T}_smoke.log
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $OUT/${T}_bench20.log 2>&1 || { tail -20 $OUT/${T}_bench20.log; exit 1; }
python -c "
import json; d=json.loads(open('$OUT/${T}_bench20.log').read().strip().splitlines()[-1])
print('bench20', d['ms_per_step']*1e3, d['roofline']['frac'], d['roofline_gather']['achieved'], d['roofline_gather']['us_per_batch'], d['per_call']['us_per_batch'], d['cpu_baseline']['value'], d['parity'])"
timeout -k 10 300 python bench.py --full --config fwfm --steps 20 --warmup 5 --no-cpu-baseline > $OUT/${T}_fwfm20.log 2>&1 || exit 1
python -c "
import json; d=json.loads(open('$OUT/${T}_fwfm20.log').read().strip().splitlines()[-1])
print('fwfm20', d['ms_per_step']*1e3, d['roofline']['frac'], d['per_call']['us_per_batch'])"
timeout -k 10 300 python tools/bench_train.py > $OUT/${T}_train.log 2>&1 || { tail -5 $OUT/${T}_train.log; exit 1; }
tail -1 $OUT/${T}_train.log
