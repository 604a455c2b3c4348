#!/bin/bash
# round 6: SKM / estimate / deferral GPU tests, a kernel trace of the whole C4 job, then the two-rank
# C4 line (bench.py --full: with its parity record) rehearsed on one GPU (super-k-mer exchange over
# gloo).  usage: bash tools/r06_a.sh   (traces and lines under $KC_OUT, default kc_out/ in the repository)
set -o pipefail
bash tools/gpu_tests.sh t2 "skm or size_table or estimate or two_processes or deferred or rehearsed" \
  tests/test_gpu_skm.py tests/test_gpu_parity.py tests/test_gpu_sharded_mp.py tests/test_gpu_defer.py \
  tests/test_bench_launch.py || exit $?
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(realpath -m "${KC_OUT:-$R/kc_out}")
mkdir -p $O
(cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_c4e -o run \
  --output-format csv -- python3 $R/bench.py --config C4 --no-cpu-baseline --no-writer --no-compact --no-cli-fullsize \
  --steps 2 --warmup 1 > $O/prof_c4e.json 2> $O/prof_c4e.err) || exit $?
python3 tools/kstats.py $O/prof_c4e/run_kernel_stats.csv > $O/prof_c4e.txt || exit $?
KC_DEFER=2 timeout -k 10 600 python3 -u bench.py --full --gpus 2 --rehearse-one-gpu --config C4 --steps 2 --warmup 1 \
  --no-cpu-baseline --no-writer --no-compact --no-cli-fullsize --multi-secondary none \
  > $O/rehearse_c4.json 2> $O/rehearse_c4.err
