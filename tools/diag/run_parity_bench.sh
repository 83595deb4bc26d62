O=${OUT:-out}; mkdir -p $O
python tools/parity_report.py fp32 > $O/parity_f64.txt 2>&1; sed -n 8,13p $O/parity_f64.txt; sed -n 16,17p $O/parity_f64.txt
python -m pytest tests/test_explorer_parity.py tests/test_explorer_fuzz_gpu.py -x -q 2>&1 | tail -3
python bench.py --full --steps 20 --warmup 5 > $O/bench_f64.txt 2>&1
python - <<PY
import json
d=json.loads(open("$O/bench_f64.txt").read().strip().splitlines()[-1])
print(d["value"], d["config"].get("stage_ms_per_step"), d["config"].get("single_graph_us"))
PY
