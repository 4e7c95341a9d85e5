# Two ranks on one GPU (gloo control plane): rehearses bench.py's multi-rank flow -- the
# driver's default `--gpus 2` command with --rehearse (every leg but the RCCL gather, which RCCL refuses on a
# shared device), the weak-scaling frames mode and the one-process group mode.
# Results go to $SF_OUT_DIR/multi/ (default bench_out/multi/).
set -e
OUT=${SF_OUT_DIR:-bench_out}/multi
mkdir -p $OUT
run() {  # run <name> <port> <bench args...>
  local name=$1 port=$2; shift 2
  timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
      --master-port $port bench.py --full --gpus 2 "$@" > $OUT/$name.json 2> $OUT/$name.err \
      || { tail -20 $OUT/$name.err; exit 1; }
  cat $OUT/$name.json
}
run dist 29517 --steps 40 --warmup 5 --rehearse
run frames 29518 --steps 20 --warmup 3 --mode frames --no-cpu-baseline --no-extras
run rows 29519 --steps 20 --warmup 3 --mode rows --no-cpu-baseline
