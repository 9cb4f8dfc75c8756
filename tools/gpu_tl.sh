# Kernel timelines of cold device-resident batches, two in flight (bench
# default), at the sizes in $TL_EVENTS.  Output $OUT/tl_<n>.txt (default
# prof_out/ in the repository root).
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-prof_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
for ev in ${TL_EVENTS:-125000 250000}; do
  rm -rf "$OUT"/tl_$ev
  timeout -k 10 300 rocprofv3 --kernel-trace -d "$OUT"/tl_$ev -o run --output-format csv -- python3 bench.py --full --no-cpu --no-extras --events $ev --steps 8 --warmup 3 > "$OUT"/tl_$ev.json 2> "$OUT"/tl.err || { tail -30 "$OUT"/tl.err; exit 1; }
  python3 tools/timeline.py "$OUT"/tl_$ev/run_kernel_trace.csv 6 > "$OUT"/tl_$ev.txt
  rm -rf "$OUT"/tl_$ev
done
