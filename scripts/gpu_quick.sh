#!/bin/bash
# GPU box: the tests named by $2 (pytest -k expression, "" = all), then a short bench line.  Usage: scripts/gpu_quick.sh <tag> [k-expr] [bench args]
tag=$1; kexpr=$2; shift; shift
out=${LOG_DIR:-logs}  # where the logs and bench lines of this run go
mkdir -p $out
if [ -n "$kexpr" ]; then
  timeout -k 10 700 python -m pytest tests -m gpu -q -k "$kexpr" > $out/${tag}_pytest.log 2>&1
else
  timeout -k 10 700 python -m pytest tests -m gpu -q > $out/${tag}_pytest.log 2>&1
fi
rc=$?
tail -12 $out/${tag}_pytest.log
if [ $rc -ne 0 ]; then echo "pytest rc=$rc: no bench"; exit $rc; fi
timeout -k 10 300 python bench.py --full --secondary 0 --cpu-evals 3 "$@" > $out/${tag}_bench.json 2> $out/${tag}_bench.err
echo "bench rc=$?"
python - <<PY
import json
try:
    r=json.loads(open('$out/${tag}_bench.json').read().strip().splitlines()[-1])
    print(round(r['ms_per_step'],5), round(r['value'],1), r.get('kernel_avg_us'), r.get('parity_on_sample'))
except Exception as e:
    print('no bench line', e)
PY
