# one GPU iteration: bash tools/gpu_iter.sh "<pytest -k expr or ALL>" [bench configs...]
# pytest (GPU tests) -> bench.py --full per config -> kernel-trace profile of the first config
# (logs and lines under $KC_OUT, default kc_out/)
set -o pipefail
K=$1; shift
OUT=${KC_OUT:-kc_out}
mkdir -p $OUT
if [ "$K" = "ALL" ]; then KARG=(); else KARG=(-k "$K"); fi
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread "${KARG[@]}" > $OUT/gpu_tests.log 2>&1 || exit 1
for c in "$@"; do
  timeout -k 10 200 python bench.py --full --config $c --no-cpu-baseline > $OUT/bench_$c.json 2> $OUT/bench_$c.err || exit 1
done
if [ $# -gt 0 ]; then bash tools/gpu_prof.sh $1 --config $1; fi
