#!/bin/bash
out=${LOG_DIR:-logs}  # where the logs and bench lines of this run go
mkdir -p $out
timeout -k 10 900 python -m pytest tests -m gpu -q > $out/r4e_pytest.log 2>&1
rc=$?; tail -30 $out/r4e_pytest.log
timeout -k 10 300 python3 scripts/drift_probe.py 2000 0.001 > $out/r4e_probe.log 2>&1
echo "probe rc=$?"; tail -22 $out/r4e_probe.log
timeout -k 10 500 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $out/r4e_bench.json 2> $out/r4e_bench.err
echo "bench rc=$?"; tail -3 $out/r4e_bench.err
python3 - <<PY
import json
for f in ("r4e_bench",):
    try:
        r=json.loads(open(f"$out/{f}.json").read().strip().splitlines()[-1])
        print(f, round(r['ms_per_step'],5), round(r['value'],1), r['n_gpus'], r.get('kernel_avg_us'), r.get('parity_on_sample'), r.get('cpu_baseline',{}).get('ms_per_eval'))
        print(' rows', {k:v for k,v in r.get('neighbour_rows').items() if 'note' not in k}); print(' drift', {k:v for k,v in r.get('drift').items() if 'note' not in k})
        for s in r.get('secondary',[]): print(' ', s['config'], round(s['ms_per_eval'],4))
        for s in r.get('other_modes',[]): print(' ', s['mode'], round(s['ms_per_eval'],4))
    except Exception as e:
        print(f, 'no line', e)
PY
