# full GPU suite, then deep packed/plain A/B (tag $1)
T=${1:-r06g}
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
[ -n "$SKIP_TESTS" ] || timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/${T}_t-all.log 2>&1 || { tail -30 $OUT/${T}_t-all.log; exit 1; }
[ -n "$SKIP_TESTS" ] || tail -2 $OUT/${T}_t-all.log
run() { # name args...
  local n=$1; shift
  timeout -k 10 250 python bench.py "$@" > $OUT/${T}_$n.log 2>&1 || { tail -5 $OUT/${T}_$n.log; exit 1; }
  python -c "
import json; d=json.loads(open('$OUT/${T}_$n.log').read().strip().splitlines()[-1])
g=d.get('roofline_gather', {})
print('$n', round(d['ms_per_step']*1e3,3), d['roofline']['frac'], g.get('achieved'), g.get('us_per_batch'), g.get('lone'), d.get('per_call', {}).get('us_per_batch'))"
}
run deep20_pk --full --steps 20 --warmup 5 --no-cpu-baseline
run deep20_plain --full --steps 20 --warmup 5 --no-cpu-baseline --pack-tables 0
run deep20_pk2 --full --steps 20 --warmup 5 --no-cpu-baseline
run deep20_plain2 --full --steps 20 --warmup 5 --no-cpu-baseline --pack-tables 0
run deep2k_pk --steps 2000 --warmup 200 --no-cpu-baseline --no-per-call
run deep2k_plain --steps 2000 --warmup 200 --no-cpu-baseline --no-per-call --pack-tables 0
