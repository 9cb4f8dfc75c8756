"""Same-box A/B of KC18 tables in the small-batch kernel (bv_kc_small_tables
on a BV_F_KEY_CACHE | BV_F_KC_COMPACT context) against the same library with
the setting off (development tool, modelled on tools/ab_small_warm.py and
tools/ab_kc_compact.py).

Workload: host batches of 1, 16, 100, 256, 512 and 1000 valid events through
bv_verify_batch on a compact context with 4, 64 or 1000 registered creators;
a batch's key table holds the keys its items name.  Per (creators, setting)
one child process: one context, every creator registered, then per batch size
5 warm-up calls and the median wall ms of 20 calls (time.perf_counter around
Verifier.verify), every status checked.  Children are interleaved over 3
rounds, each under a time limit; the run stops at the first failed child.

  off   bv_kc_small_tables(ctx, 0), the state after bv_create: cold k_small
        up to 256 items, the bulk KC18 pipeline above.  The BASELINE.
  on    bv_kc_small_tables(ctx, 1): k_small<18, 8> on the tables up to 1024
        fully cached items.

  python tools/ab_kc18_small.py [--out profiles/kc18_small_ab.json]

Every figure goes to the JSON file, rewritten after each child.  The summary
holds, per cell, both settings' median / min / max over the rounds and
`wins`: the on median is below the off median by more than the off setting's
own spread (max - min) over the rounds.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 16, 100, 256, 512, 1000)
WARMUP, CALLS = 5, 20
CHILD_LIMIT_S = 240


def used_keys_only(b):
    import numpy as np

    from babble_amd.batch import PackedBatch

    used, inv = np.unique(b.item_key, return_inverse=True)
    keys = [b.key(int(k)) for k in used]
    off = np.zeros(len(keys) + 1, np.uint64)
    off[1:] = np.cumsum([len(k) for k in keys])
    kb = np.frombuffer(b"".join(keys), np.uint8).copy()
    return PackedBatch(b.msg_bytes, b.msg_off, kb, off, b.item_msg, inv.astype(np.uint32), b.r_be, b.s_be, b.pre)


def child():
    sys.path.insert(0, ROOT)
    from babble_amd import native, synth
    from babble_amd.verifier import Verifier

    on, n_creators = os.environ["AB_SETTING"] == "on", int(os.environ["AB_CREATORS"])
    everyone = synth.events(max(n_creators, 1000), n_creators=n_creators, seed=2)
    keys = sorted({everyone.key(k) for k in range(everyone.n_keys)})
    assert len(keys) == n_creators
    v = Verifier(0, flags=native.F_KEY_CACHE | native.F_KC_COMPACT)
    t0 = time.perf_counter()
    v.register_keys(keys)
    out = {"register_s": time.perf_counter() - t0, "sizes": {}}
    assert v.timing()["kc_keys"] == n_creators, v.timing()
    v.kc_small_tables(on)
    for n in SIZES:
        b = used_keys_only(synth.events(n, n_creators=n_creators, seed=2))
        assert set(b.key(k) for k in range(b.n_keys)) <= set(keys)
        ms = []
        for k in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            res = v.verify(b)
            el = (time.perf_counter() - t0) * 1e3
            assert int((res.status == native.ACCEPT).sum()) == n, (n, k)
            if k >= WARMUP:
                ms.append(el)
        t = v.timing()
        out["sizes"][str(n)] = {"ms": statistics.median(ms), "ms_min": min(ms), "key_path": t["key_path"],
                                "kc_hits": t["kc_hits"], "small_path": t["ms_h2d"] == 0, "ms_kernel": t["ms_total"]}
    v.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kc18_small_ab.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--creators", default="4,64,1000")
    a = ap.parse_args()
    creators = [int(x) for x in a.creators.split(",")]
    res = {"rounds": a.rounds, "warmup": WARMUP, "calls": CALLS, "unit": "median wall ms per bv_verify_batch call",
           "baseline": "off: the same library, bv_kc_small_tables(ctx, 0)", "runs": {}, "summary": {}}
    for rnd in range(a.rounds):
        for c in creators:
            for setting in ("off", "on"):
                env = dict(os.environ, AB_CHILD="1", AB_SETTING=setting, AB_CREATORS=str(c))
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True,
                                       text=True, timeout=CHILD_LIMIT_S)
                except subprocess.TimeoutExpired:
                    print(c, setting, "ran past its time limit", flush=True)
                    sys.exit(1)
                line = [x for x in p.stdout.splitlines() if x.startswith("{")]
                if p.returncode != 0 or not line:
                    print(c, setting, "failed", p.returncode, p.stderr[-2000:], flush=True)
                    sys.exit(1)
                r = json.loads(line[-1])
                res["runs"].setdefault(str(c), {}).setdefault(setting, []).append(r)
                print(f"round {rnd} creators {c:4d} {setting:3s} register {r['register_s']:.2f} s  " + "  ".join(
                    f"{n}: {r['sizes'][str(n)]['ms']:.3f}" for n in SIZES), flush=True)
                if setting == "on":
                    cell = res["summary"].setdefault(str(c), {})
                    for n in SIZES:
                        s = {}
                        for name in ("off", "on"):
                            runs = [x["sizes"][str(n)] for x in res["runs"][str(c)][name]]
                            vals = [x["ms"] for x in runs]
                            s[name] = {"median": statistics.median(vals), "min": min(vals), "max": max(vals),
                                       "key_path": runs[-1]["key_path"], "small_path": runs[-1]["small_path"]}
                        s["off_spread"] = s["off"]["max"] - s["off"]["min"]
                        s["wins"] = s["off"]["median"] - s["on"]["median"] > s["off_spread"]
                        cell[str(n)] = s
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1, sort_keys=True)
                    f.write("\n")
    for c, cell in res["summary"].items():
        for n, s in cell.items():
            print(f"creators {c:>4s} items {n:>4s}  off {s['off']['median']:.3f} ms [{s['off']['min']:.3f}, "
                  f"{s['off']['max']:.3f}] (path {s['off']['key_path']})  on {s['on']['median']:.3f} ms "
                  f"[{s['on']['min']:.3f}, {s['on']['max']:.3f}] (path {s['on']['key_path']})  "
                  f"{'wins' if s['wins'] else 'DOES NOT WIN'}", flush=True)


if __name__ == "__main__":
    if os.environ.get("AB_CHILD"):
        child()
        sys.exit(0)
    main()
