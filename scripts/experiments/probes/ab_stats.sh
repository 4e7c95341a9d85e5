# rocprofv3 kernel stats: bench with SF_ORDER=0 vs 1, and the tile_schedule script (4 renders)
# Results go to $SF_OUT_DIR/ab/ (default bench_out/ab/).
set -e
R=$PWD
export AB=$R/${SF_OUT_DIR:-bench_out}/ab
mkdir -p $AB
cd /tmp && export TMPDIR=/tmp
for O in 0 1; do
  SF_ORDER=$O timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $AB/o$O -o run --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline --steps 30 --warmup 5 > $AB/o$O.log 2>&1
  echo "== SF_ORDER=$O"; grep -h "sf_" $(find $AB/o$O -name "*kernel_stats.csv")
done
timeout -k 10 300 rocprofv3 --kernel-trace -d $AB/ts -o run --output-format csv -- python3 $R/scripts/tile_schedule.py --out $AB/tt.npy > $AB/ts.log 2>&1
python3 - <<'PY'
import csv,glob,os
f=glob.glob(os.environ['AB']+'/ts/**/*kernel_trace.csv',recursive=True)[0]
for r in csv.DictReader(open(f)):
    if r['Kernel_Name'].startswith('sf_'): print(r['Kernel_Name'], (int(r['End_Timestamp'])-int(r['Start_Timestamp']))/1e3, 'us')
PY
