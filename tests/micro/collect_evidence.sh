#!/bin/bash
# everything profiles/rNN_* is made of, in one call on the GPU box (repo root): bench lines of the four workloads, rocprofv3 stats + PMC
# passes of the headline bench (profile_bench.sh), plugin path rates -> $OUT_ROOT/evidence (OUT_ROOT defaults to tests/micro/_out)
set -e
R=${1:-r03}
export OUT_ROOT=${OUT_ROOT:-tests/micro/_out}
EV=$OUT_ROOT/evidence
mkdir -p $EV
python3 bench.py --full --docbytes 65536 > $EV/${R}_bench_line.json 2> $EV/bench.err || { tail -5 $EV/bench.err; exit 1; }
python3 bench.py --full --workload lexer --no-cpu-baseline > $EV/${R}_bench_line_lexer.json 2>> $EV/bench.err
python3 bench.py --full --workload l2 > $EV/${R}_bench_line_l2.json 2>> $EV/bench.err
timeout -k 10 300 python3 bench.py --full --workload trees --no-cpu-baseline > $EV/${R}_bench_line_trees.json 2>> $EV/bench.err || echo "trees bench failed"
timeout -k 10 300 python3 tests/micro/plugin_threads.py 64 16384 1,4,8,16 > $EV/${R}_plugin_threads.txt 2>&1 || true; cat $EV/${R}_plugin_threads.txt
bash tests/micro/profile_bench.sh > $EV/profile_bench.log 2>&1 || { tail -20 $EV/profile_bench.log; exit 1; }
cp $OUT_ROOT/prof_bench/summary.json $EV/${R}_bench_pmc_summary.json
cp $OUT_ROOT/prof_bench/kernel_stats.csv $EV/${R}_bench_kernel_stats.csv
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT_ROOT/prof_trees --output-format csv -- python3 bench.py --full --workload trees --no-cpu-baseline --steps 2 > $EV/trees_prof.log 2>&1 || true
cp $(ls $OUT_ROOT/prof_trees/*/*kernel_stats.csv | head -1) $EV/${R}_trees_kernel_stats.csv || true
tail -c 600 $EV/${R}_bench_line.json; echo; cat $EV/${R}_plugin_threads.txt; tail -8 $EV/profile_bench.log
