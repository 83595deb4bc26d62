#!/bin/bash
# Run ON THE GPU BOX right after tools/profile_round.sh: text summaries of the rocprofv3 databases (the .db files are
# too large to keep), HBM traffic file, parity table.
R=$PWD
O=${OUT:-$R/out}
python tools/rocprof_summary.py $(find $O/trace -name "*.db" | head -1) $O/kernel_stats.txt > /dev/null 2>&1
python tools/pmc_summary.py $(find $O/pmc_fetch $O/pmc_write $O/pmc_sq -name "*.db") -o $O/pmc_counters.txt > /dev/null 2>&1
python tools/traffic_json.py $(find $O/pmc_fetch $O/pmc_write -name "*.db") > $O/traffic.log 2>&1   # round 3: tools/profile_r03.sh is the current script
cp profiles/kernel_traffic.json $O/
python tools/parity_report.py > $O/parity.txt 2>&1
find $O -name "*.db" -delete
ls $O
