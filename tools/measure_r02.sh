#!/bin/bash
# Round-2 measurement in one command on a GPU machine, everything to $OUT (default measure_out):
#   default bench line, rocprofv3 --kernel-trace --stats of the same command, three separate --pmc passes
#   (MFMA busy / FETCH_SIZE / WRITE_SIZE: TCC counters do not fit one pass), per-kernel summary.
# rocprofv3 gets the program itself after `--` (python ...): no env / bash -c hop (the profiler initialises the GPU).
set -o pipefail
R=$PWD; OUT=${OUT:-measure_out}; mkdir -p $OUT; OUT=$(cd $OUT && pwd)
timeout -k 10 500 python bench.py --full > $OUT/r02_bench.json 2> $OUT/r02_bench.err || { echo "bench failed"; tail -5 $OUT/r02_bench.err; exit 1; }
tail -14 $OUT/r02_bench.err; cat $OUT/r02_bench.json
DSX_BENCH_OPS=$OUT/r02_ops.json timeout -k 10 300 python bench.py --full --steps 200 --warmup 5 --no-cpu-baseline > $OUT/r02_bench200.json 2> $OUT/r02_bench200.err || exit 1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r02_prof -- python $R/bench.py --steps 200 --warmup 5 --no-cpu-baseline --no-roofline > $OUT/r02_prof.log 2>&1 || { echo "rocprof stats failed"; exit 1; }
timeout -k 10 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVES GRBM_GUI_ACTIVE --output-format csv -d $OUT/r02_pmc_mfma -- python $R/bench.py --steps 3 --warmup 1 --no-graph --no-cpu-baseline --no-roofline > $OUT/r02_pmc_mfma.log 2>&1 || { echo "pmc mfma failed"; exit 1; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/r02_pmc_fetch -- python $R/bench.py --steps 3 --warmup 1 --no-graph --no-cpu-baseline --no-roofline > $OUT/r02_pmc_fetch.log 2>&1 || { echo "pmc fetch failed"; exit 1; }
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/r02_pmc_write -- python $R/bench.py --steps 3 --warmup 1 --no-graph --no-cpu-baseline --no-roofline > $OUT/r02_pmc_write.log 2>&1 || { echo "pmc write failed"; exit 1; }
cd $R
python tools/pmc_summary.py $OUT/r02_pmc_mfma $OUT/r02_pmc_fetch $OUT/r02_pmc_write $OUT/r02_ops.json $OUT/r02_counters.json > $OUT/r02_pmc_summary.txt 2>&1; tail -40 $OUT/r02_pmc_summary.txt
find $OUT/r02_prof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/r02_kernel_stats.csv
