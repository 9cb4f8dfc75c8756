"""Same-box A/B of the compact key-cache tier (BV_F_KC_COMPACT, KC18 tables)
against the parent commit's library (development tool, modelled on
tools/ab_kc.py).

Workload: resident C2 events, two batches in flight as bench.py's `warm` leg,
verifies/s over 40 steps.  1M events at 64, 200 and 1000 creators, and 128k
events at 1000 creators.  Variants, each in its own child process, interleaved
over 3 rounds, a time limit per child, stop at the first failed child:

  parent/default   the parent commit's library, per-batch tables (F_DEFAULT)
  parent/kc22      the parent commit's library, 22-bit cache (64 creators only:
                   the default budget holds 119 tables)
  new/kc18         this library, F_KEY_CACHE | F_KC_COMPACT (all keys registered;
                   the registration's wall time is recorded)
  new/default      this library on the two parent variants: they must not move
  new/kc22

  python tools/ab_kc_compact.py --parent-lib PATH/libbabbleverify.so [--out profiles/kc_compact_ab.json]

The baseline of every comparison is the parent's library in the same run on
the same box.  Every figure goes to the JSON file, rewritten after each child.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 40
CHILD_LIMIT_S = 240


def child():
    sys.path.insert(0, ROOT)
    import torch

    from babble_amd import native, synth

    if os.environ.get("AB_LIB"):
        native.LIB_PATH = os.path.abspath(os.environ["AB_LIB"])
        native._lib = None
    from babble_amd.verifier import Verifier

    mode = os.environ["AB_MODE"]
    n_events, n_creators = int(os.environ["AB_EVENTS"]), int(os.environ["AB_CREATORS"])
    flags = {"default": native.F_DEFAULT, "kc22": native.F_KEY_CACHE,
             "kc18": native.F_KEY_CACHE | native.F_KC_COMPACT}[mode]
    b = synth.events(n_events, n_creators=n_creators, seed=2)
    v = Verifier(0, flags=flags)
    out = {}
    if mode != "default":
        t0 = time.perf_counter()
        v.register_keys([b.key(k) for k in range(b.n_keys)])
        out["register_s"] = time.perf_counter() - t0
        t = v.timing()
        out["kc_builds"], out["kc_keys"] = t["kc_builds"], t["kc_keys"]
        assert t["kc_keys"] == n_creators, t
    ds = [v.to_device(b) for _ in range(2)]
    for k in range(4):
        v.verify_device(ds[k % 2], stream=0, sync=False)
    torch.cuda.synchronize()
    v.sync()
    t0 = time.perf_counter()
    for k in range(STEPS):
        v.verify_device(ds[k % 2], stream=0, sync=False)
    v.sync()
    el = time.perf_counter() - t0
    spans, keyprep = [], []
    for _ in range(3):
        v.verify_device(ds[0], sync=True)
        t = v.timing()
        spans.append(t["ms_total"])
        keyprep.append(t["ms_keyprep"])
    out["key_path"] = t["key_path"]
    assert int((ds[0].result().status == 1).sum()) == b.n_items
    assert int((ds[1].result().status == 1).sum()) == b.n_items
    v.close()
    out.update(value=b.n_items * STEPS / el, ms_total_alone=min(spans), ms_keyprep_alone=min(keyprep))
    print(json.dumps(out), flush=True)


def summarise(runs):
    vals = [r["value"] for r in runs]
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals), "n": len(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libbabbleverify.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kc_compact_ab.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="1000000x64,1000000x200,1000000x1000,131072x1000")
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_lib)
    if not os.path.exists(parent):
        sys.exit(f"{parent}: no such library")
    jobs = []  # (shape, variant, lib, mode)
    for shape in a.shapes.split(","):
        n_events, n_creators = (int(x) for x in shape.split("x"))
        variants = [("parent/default", parent, "default"), ("new/kc18", "", "kc18"), ("new/default", "", "default")]
        if n_creators <= 119:  # what the 805 MB tables hold at the default budget
            variants += [("parent/kc22", parent, "kc22"), ("new/kc22", "", "kc22")]
        jobs += [(shape, n_events, n_creators, name, lib, mode) for name, lib, mode in variants]
    res = {"steps": STEPS, "rounds": a.rounds, "workload": "resident C2 events, two batches in flight",
           "unit": "verifies/s", "runs": {}, "summary": {}}
    for rnd in range(a.rounds):
        for shape, n_events, n_creators, name, lib, mode in jobs:
            env = dict(os.environ, AB_CHILD="1", AB_LIB=lib, AB_MODE=mode, AB_EVENTS=str(n_events),
                       AB_CREATORS=str(n_creators))
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True,
                                   text=True, timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(shape, name, "ran past its time limit", flush=True)
                sys.exit(1)
            line = [x for x in p.stdout.splitlines() if x.startswith("{")]
            if p.returncode != 0 or not line:
                print(shape, name, "failed", p.returncode, p.stderr[-2000:], flush=True)
                sys.exit(1)
            r = json.loads(line[-1])
            res["runs"].setdefault(shape, {}).setdefault(name, []).append(r)
            res["summary"].setdefault(shape, {})[name] = summarise(res["runs"][shape][name])
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1, sort_keys=True)
                f.write("\n")
            reg = f"  register {r['register_s']:.2f} s" if "register_s" in r else ""
            print(f"round {rnd} {shape:>13s} {name:15s} {r['value'] / 1e6:7.1f} M/s  key_path {r['key_path']:2d}  "
                  f"alone {r['ms_total_alone']:.3f} ms{reg}", flush=True)
    for shape, by in res["summary"].items():
        base = by["parent/default"]
        spread = base["max"] - base["min"]
        for name, s in by.items():
            print(f"{shape:>13s} {name:15s} median {s['median'] / 1e6:7.1f} M/s  [{s['min'] / 1e6:.1f}, "
                  f"{s['max'] / 1e6:.1f}]  vs parent/default {(s['median'] - base['median']) / 1e6:+.1f} M/s "
                  f"(its spread {spread / 1e6:.1f})", flush=True)


if __name__ == "__main__":
    if os.environ.get("AB_CHILD"):
        child()
        sys.exit(0)
    main()
