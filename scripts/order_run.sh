# every config in a process of its own, then the --full run that times them all in one process
#   bash scripts/order_run.sh OUTDIR
set -e
out=${1:?usage: order_run.sh OUTDIR}
mkdir -p "$out"
for c in fill slots receive segment c3 c4 c5; do
  timeout -k 10 300 python bench.py --full --config $c --no-cpu-baseline --no-e2e > "$out/alone_$c.log" 2>&1
done
timeout -k 10 400 python bench.py --full --no-cpu-baseline --no-e2e > "$out/order_default.log" 2>&1
