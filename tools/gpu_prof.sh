# rocprofv3 kernel-trace summary of the bench (no CPU leg).  Output goes to
# $OUT (default prof_out/ in the repository root).
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-prof_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
rm -rf "$OUT"/prof
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT"/prof -o run --output-format csv -- python3 bench.py --full --no-cpu --no-extras --steps 5 --warmup 2 ${BENCH_ARGS:-} > "$OUT"/bench_prof.json 2> "$OUT"/prof.err || { tail -30 "$OUT"/prof.err; exit 1; }
cat "$OUT"/bench_prof.json
python3 - "$OUT"/prof/run_kernel_stats.csv <<'PY'
import csv, sys
rows=list(csv.DictReader(open(sys.argv[1])))
for r in rows:
    print(f"{r['Name'].split('(')[0][:60]:60s} calls={r['Calls']:>4s} avg_us={float(r['AverageNs'])/1e3:9.1f}")
PY
