#!/bin/bash
# round 5, first GPU pass: new tests, census, planner parity (incl. bf16 decision level), bench line
O=${OUT:-out/r05}
mkdir -p $O
python -m pytest tests/test_status_gpu.py tests/test_dist_gpu.py -x -q > $O/tests_new.log 2>&1
echo "tests_new rc=$?" >> $O/tests_new.log
python bench.py --full > $O/bench.json 2> $O/bench.err
python tools/parity_census.py > $O/parity_census.txt 2>&1
python tools/planner_parity.py > $O/planner_parity.txt 2>&1
tail -5 $O/tests_new.log
