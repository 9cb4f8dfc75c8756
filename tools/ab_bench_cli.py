"""Same-box A/B of library variants (tools/build_variant.sh) through bench.py
itself (development tool): per round, each variant's .so is copied over
babble_amd/libbabbleverify.so and bench.py runs as its own process, so the
variants alternate and clock drift hits all of them alike; the tree's own
library is put back at the end.  A failing run ends the script.

    python tools/ab_bench_cli.py OUTLOG ROUNDS name=lib.so ... [-- bench.py args]

With AB_DUMP=DIR the first round also passes --dump-outputs DIR/<name>."""
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.chdir(root)
args = sys.argv[1:]
extra = []
if "--" in args:
    k = args.index("--")
    args, extra = args[:k], args[k + 1:]
outlog, rounds = args[0], int(args[1])
variants = [a.split("=", 1) for a in args[2:]]
dst = os.path.join(root, "babble_amd", "libbabbleverify.so")
keep = dst + ".keep"
shutil.copy(dst, keep)
res = {n: [] for n, _ in variants}
raw = []
dump = os.environ.get("AB_DUMP")  # dump outputs of the first round into AB_DUMP/<name>
try:
    for rnd in range(1, rounds + 1):
        for name, lib in variants:
            shutil.copy(lib, dst)
            cmd = [sys.executable, "bench.py", "--gpus", "1"] + extra
            if dump and rnd == 1:
                cmd += ["--dump-outputs", os.path.join(dump, name)]
            t0 = time.time()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print("FAILED", name, rnd, r.returncode, r.stdout[-1500:], r.stderr[-3000:], flush=True)
                sys.exit(1)
            line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
            j = json.loads(line)
            res[name].append((j["value"], j["ms_per_step"]))
            raw.append(f"{name} {rnd} {line}")
            print(rnd, name, round(j["value"] / 1e6, 3), round(j["ms_per_step"], 4), f"{time.time() - t0:.1f}s", flush=True)
finally:
    shutil.copy(keep, dst)
    os.remove(keep)
with open(outlog, "w") as f:
    f.write(f"# same-box A/B through bench.py {' '.join(extra)}: {', '.join(n for n, _ in variants)}; {rounds} alternating rounds\n")
    for k, lab, sc in ((0, "value_M", 1e-6), (1, "ms_per_step", 1.0)):
        for name, _ in variants:
            v = [x[k] * sc for x in res[name]]
            f.write(f"ab_plain {lab:<14} {name:<8} median {statistics.median(v):10.4f} min {min(v):10.4f} max {max(v):10.4f} "
                    f"spread {max(v) - min(v):8.4f}  runs {' '.join(f'{x:.4f}' for x in v)}\n")
    f.write("\n# raw result lines (variant round json)\n" + "\n".join(raw) + "\n")
print(open(outlog).read().split("\n# raw")[0])
