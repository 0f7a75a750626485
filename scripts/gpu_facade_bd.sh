# writes under $OUT (default bench_out/facade_bd)
export TMPDIR=/tmp
OUT=${OUT:-bench_out/facade_bd}
mkdir -p $OUT
for m in walk iter walk iter; do
timeout -k 10 200 python scripts/facade_workload.py 65536 1000 3 250 $m >> $OUT/facade_workload_$m.jsonl 2>&1 || exit $?
done
timeout -k 10 200 python bench.py --full --steps 1000 --warmup 250 --no-cpu-baseline --no-launched > $OUT/bench_replay.jsonl 2>&1 || exit $?
