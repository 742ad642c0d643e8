#!/bin/bash
# Round-end measurement on a GPU machine: full GPU tests, the --full bench line, rocprofv3 kernel stats, HBM traffic (PMC).
# Everything goes to $OUT (default measure_out).
set -o pipefail
R=$PWD; OUT=${OUT:-measure_out}; mkdir -p $OUT; OUT=$(cd $OUT && pwd)
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $OUT/final_tests.log 2>&1; echo "tests rc=$?" | tee -a $OUT/final_tests.log
tail -3 $OUT/final_tests.log
timeout -k 10 400 python bench.py --full > $OUT/final_bench.json 2> $OUT/final_bench.err; echo "bench rc=$?"
tail -12 $OUT/final_bench.err
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final_prof -- python $R/bench.py --steps 200 --warmup 5 --no-cpu-baseline --no-roofline > $OUT/final_prof.log 2>&1; echo "rocprof rc=$?"
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/final_pmc_fetch -- python $R/bench.py --steps 3 --warmup 1 --no-graph --no-cpu-baseline --no-roofline > $OUT/final_pmc_fetch.log 2>&1; echo "pmc fetch rc=$?"
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/final_pmc_write -- python $R/bench.py --steps 3 --warmup 1 --no-graph --no-cpu-baseline --no-roofline > $OUT/final_pmc_write.log 2>&1; echo "pmc write rc=$?"
cd $R; ls $OUT/final_prof/*/ $OUT/final_pmc_fetch/*/ | head
