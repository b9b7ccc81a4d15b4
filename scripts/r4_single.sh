#!/bin/bash
out=${LOG_DIR:-logs}  # where the logs and bench lines of this run go
mkdir -p $out
timeout -k 10 600 python -m pytest tests/test_gpu_parity.py -m gpu -q -x -k "single or fast" > $out/r4r_pytest.log 2>&1
rc=$?; tail -15 $out/r4r_pytest.log
for m in fast fast+single; do
  for i in 1 2; do
  timeout -k 10 180 python bench.py --full --steps 300 --cpu-evals 3 --secondary 0 --mode $m 2> $out/r4r_$m.err | python -c "
import sys, json
d = json.loads([l for l in sys.stdin.read().strip().split('\n') if l.startswith('{')][-1])
print('$m', round(d['ms_per_step'] * 1e3, 2), d['kernel_avg_us'], d.get('parity_on_sample'))"
  done
done
