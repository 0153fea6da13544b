set -e
OUT=${OUT:-build/out}  # where the logs and result lines go
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gpu_tests_st.log 2>&1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_st.log 2>&1
timeout -k 10 300 python bench.py --full > $OUT/bench_st.log 2>&1
for c in 3 1 5; do
  timeout -k 10 120 python bench.py --full --config $c --steps 20 --no-cpu-baseline --no-e2e > $OUT/stc_$c.log 2>&1
done
