#!/bin/bash
# round 6: kind 7 closes once per step — kind-7 and DES parity, the kind-7
# bench lines, a timing A/B against the round's start, c4 / c3p / c3s profiles
set -o pipefail
cd $GRAFT_REPO_ROOT && mkdir -p gpurun_out/r6k
O=gpurun_out/r6k
timeout -k 10 800 python -u -m pytest -x -q --timeout 400 --timeout-method thread -m gpu \
  tests/test_walk_gpu.py tests/test_kat_gpu.py tests/test_golden_records_gpu.py tests/test_fullsize_gpu.py \
  tests/test_des_items_gpu.py > $O/tests.log 2>&1
rc=$?
tail -2 $O/tests.log
[ $rc -eq 0 ] || { grep -E "FAILED|Error" $O/tests.log | head; exit $rc; }
for c in c4 c3p c3s c4w cdag; do
timeout -k 10 600 python bench.py --full --config $c > $O/bench_$c.log 2>&1 || { tail -20 $O/bench_$c.log; exit 6; }
grep '^{' $O/bench_$c.log | tail -1 | python -c "import json,sys;d=json.loads(sys.stdin.read());print('$c', d['value'], d['roofline']['kernel_ms'], d.get('speedup_vs_wave_walk'))"
done
SETS="c4|--config_c4 c3p|--config_c3p c3s|--config_c3s" bash tools/gpu_r6_prof.sh
