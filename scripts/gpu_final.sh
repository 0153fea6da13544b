#!/bin/bash
# final check on the committed code: smoke, GPU suite, default bench line
export TMPDIR=/tmp
OUT=${OUT:-build/out}  # where the logs and result lines go
mkdir -p "$OUT"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/final_smoke.log 2>&1 || { tail -20 $OUT/final_smoke.log; exit 1; }
tail -1 $OUT/final_smoke.log
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/final_tests.log 2>&1 || { tail -30 $OUT/final_tests.log; exit 1; }
tail -1 $OUT/final_tests.log
timeout -k 10 300 python bench.py --full > $OUT/final_bench.json 2> $OUT/final_bench.err || { tail $OUT/final_bench.err; exit 1; }
python -c "import json; d=json.load(open('$OUT/final_bench.json')); print(d['value'], d['ms_per_step'], d['roofline'], d['cpu_baseline'])"
