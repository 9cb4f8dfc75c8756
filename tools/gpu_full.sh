# Full GPU pass: pytest -m gpu, smoke, the full bench line (bench.py --full),
# rocprofv3 kernel stats of the headline (one batch in flight), then optional
# extra steps ($FULL_EXTRA, a command).  Output goes to $OUT (default prof_out/
# in the repository root).  Each step limited; a failing step ends the script.
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-prof_out}
mkdir -p "$OUT"
echo "box $(hostname)"
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > "$OUT"/pytest_gpu.log 2>&1 || { echo PYTEST FAILED; tail -60 "$OUT"/pytest_gpu.log; exit 1; }
tail -2 "$OUT"/pytest_gpu.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke.log 2>&1 || { echo SMOKE FAILED; tail -30 "$OUT"/smoke.log; exit 1; }
tail -3 "$OUT"/smoke.log
timeout -k 10 400 python -u bench.py --full > "$OUT"/bench.json 2> "$OUT"/bench.err || { echo BENCH FAILED; tail -30 "$OUT"/bench.err; exit 1; }
python3 -c "import json, sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('bench', round(d['value']/1e6,1), 'M/s', d['roofline']['frac'])" "$OUT"/bench.json
rm -rf "$OUT"/prof
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT"/prof -o run --output-format csv -- python3 bench.py --full --no-cpu --no-extras --inflight 1 --steps 5 --warmup 2 > "$OUT"/bench_prof.json 2> "$OUT"/prof.err || { tail -30 "$OUT"/prof.err; exit 1; }
cp "$OUT"/prof/run_kernel_stats.csv "$OUT"/bench_kernel_stats.csv
rm -rf "$OUT"/prof
if [ -n "$FULL_EXTRA" ]; then eval "$FULL_EXTRA"; fi
