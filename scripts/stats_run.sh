# Kernel-trace profile of a short bench run (rocprofv3 --kernel-trace --stats); summary to $SF_OUT_DIR/<tag>/
# (default bench_out/<tag>/)
set -e
T=${1:-stats}
R=$PWD
OUT=$R/${SF_OUT_DIR:-bench_out}/$T
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline --steps 30 --warmup 5 > $OUT/bench.log 2>&1
cat $(find $OUT/prof -name "*kernel_stats.csv")
tail -1 $OUT/bench.log
