# SQ_INSTS_VALU of library variants (tools/build_variant.sh) over the bench
# workload: one rocprofv3 --pmc run per variant, nothing else traced, the
# variant's library copied over babble_amd/libbabbleverify.so for its run and
# the tree's own put back after it.  Output: $OUT/pmcab_<name>/ (default
# prof_out/), summarised per kernel by tools/pmc_ab_summary.py $OUT.
#     tools/gpu_pmc_ab.sh parent=variants/parent.so y3=variants/y3.so ...
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-prof_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
EV=${PMC_EVENTS:-1000000}
keep=$(mktemp)
cp babble_amd/libbabbleverify.so "$keep" || exit 1
for arg in "$@"; do
  name=${arg%%=*}; lib=${arg#*=}
  cp "$lib" babble_amd/libbabbleverify.so || exit 1
  timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_VALU -d "$OUT"/pmcab_$name -o run --output-format csv -- \
    python3 bench.py --full --no-cpu --no-extras --inflight 1 --steps 2 --warmup 1 --events $EV > "$OUT"/pmcab_$name.log 2>&1
  rc=$?
  cp "$keep" babble_amd/libbabbleverify.so
  if [ $rc -ne 0 ]; then echo "PMC pass $name failed (rc $rc)"; tail -20 "$OUT"/pmcab_$name.log; rm -f "$keep"; exit 1; fi
  echo "pass $name ok"
done
rm -f "$keep"
python3 tools/pmc_ab_summary.py "$OUT"
