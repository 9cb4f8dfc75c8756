"""Rehearsal of bv_group_verify_events on one GPU (development tool): 1M C2
bulk events (every parent a known hash) from pinned memory through

    verifier   Verifier.verify_events_into (one context, the un-based kernels)
    group1     Group([0]).verify_events_into           (plan + gather only)
    group2     Group([0, 0]).verify_events_into        (2 logical shards)
    group4     Group([0, 0, 0, 0]).verify_events_into  (4 logical shards)
    parent     (--parent-lib PATH) bv_verify_events of ANOTHER build of the
               library, e.g. the parent commit's, from its own pinned arena

The variants alternate call by call in one process (so clocks, thermals and
other tenants' load hit them alike), in an order rotated every round; after
a warm-up each gets --calls timed calls (>= 20); median and min-max per
variant, every call's time, the device-side breakdown of each `verifier`
call, and the spread of the baseline's own repeats (the parent library's
when given, else `verifier`'s).  --variants runs a subset (e.g. `verifier`
alone beside the parent library).  The last result of every variant is
checked against the seeded rejections.  Logical shards share one GPU: group2
/ group4 rehearse the multi-device code path and are recorded, not expected
to be faster; no multi-device figure is measured here.
Writes profiles/group_events_rehearsal.json (--out).  Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from babble_amd import native, synth  # noqa: E402
from babble_amd.verifier import Group, PinnedArena, Verifier, VerifyResult  # noqa: E402


class OtherLib:
    """bv_verify_events of a second build of the library beside this one
    (only the symbols the parent commit already has), with its own arena:
    each build DMAs in place only from its own bv_host_alloc memory."""

    def __init__(self, path):
        P = ctypes.c_void_p
        L = self._L = ctypes.CDLL(os.path.abspath(path))
        L.bv_create.argtypes = [ctypes.POINTER(P), ctypes.c_int, ctypes.c_uint32]
        L.bv_destroy.argtypes = [P]
        L.bv_last_error.argtypes = [P]
        L.bv_last_error.restype = ctypes.c_char_p
        L.bv_verify_events.argtypes = [P, P, ctypes.POINTER(native.BvResult)]
        L.bv_host_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(P)]
        L.bv_host_free.argtypes = [P]
        L.bv_host_free.restype = None
        self.ctx = P()
        rc = L.bv_create(ctypes.byref(self.ctx), 0, 0)
        if rc != native.BV_OK:
            raise native.BvError(rc, "bv_create (other library)")
        self.arena = PinnedArena(lib=L)

    def verify_events_into(self, eb, res):
        keep = []
        cb = eb.c_struct(keep)
        r = native.BvResult(res.msg_hash.ctypes.data, res.status.ctypes.data, res.accept_bits.ctypes.data)
        rc = self._L.bv_verify_events(self.ctx, ctypes.byref(cb), ctypes.byref(r))
        if rc != native.BV_OK:
            raise native.BvError(rc, self._L.bv_last_error(self.ctx).decode(errors="replace"))
        return res

    def close(self):
        self._L.bv_destroy(self.ctx)
        self.arena.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variants", default="verifier,group1,group2,group4",
                    help="which of verifier, group1, group2, group4 to run (the full set is the rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_events_rehearsal.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("group_events_rehearsal: no GPU")
    if a.calls < 20:
        sys.exit("group_events_rehearsal: at least 20 timed calls per variant")
    n = a.events
    _, wire = synth.event_fields(n, n_creators=64, seed=2, parents="hash")
    bad = np.random.default_rng(2).choice(n, size=max(1, n // 1000), replace=False)
    wire.s_be[bad, 5] ^= 0x20  # the seeded rejections
    want = np.ones(n, np.uint8)
    want[bad] = 0
    want_bits = np.packbits(want, bitorder="little")
    want_bits = np.concatenate([want_bits, np.zeros(-len(want_bits) % 8, np.uint8)]).view(np.uint64)

    arena = PinnedArena()
    pw = arena.wire(wire)

    def results(ar):
        return VerifyResult(ar.array((n, 32), np.uint8), ar.array(n, np.uint8), ar.array((n + 63) // 64, np.uint64))

    make = {"verifier": lambda: Verifier(0), "group1": lambda: Group([0]), "group2": lambda: Group([0, 0]),
            "group4": lambda: Group([0, 0, 0, 0])}
    handles = {k: make[k]() for k in a.variants.split(",")}
    variants = {k: (h, pw, results(arena)) for k, h in handles.items()}
    if a.parent_lib:
        other = handles["parent"] = OtherLib(a.parent_lib)
        variants["parent"] = (other, other.arena.wire(wire), results(other.arena))
    order = sorted(variants)
    ts = {k: [] for k in order}
    breakdown = []
    for it in range(a.warmup + a.calls):
        # the round's order is rotated, so every variant runs equally often in
        # every position (after every other variant)
        for k in order[it % len(order):] + order[: it % len(order)]:
            h, w, r = variants[k]
            t0 = time.perf_counter()
            h.verify_events_into(w, r)
            dt = (time.perf_counter() - t0) * 1e3
            if it >= a.warmup:
                ts[k].append(dt)
                if k == "verifier":  # the device-side breakdown of each of its calls
                    tm = h.timing()
                    breakdown.append({f: round(tm[f], 3) for f in ("ms_total", "ms_h2d", "ms_host_prep", "ms_sha256",
                                                                  "ms_verify", "ms_host")})
    ref = variants[order[0]][2]
    for k in order:  # the last result of each variant against the seeded rejections
        r = variants[k][2]
        assert np.array_equal(r.status, want), k
        assert np.array_equal(r.accept_bits, want_bits), k
        assert np.array_equal(r.msg_hash, ref.msg_hash), k
    out = {"events": n, "calls": a.calls, "warmup": a.warmup, "rejections": int(len(bad)),
           "device": torch.cuda.get_device_name(0),
           "method": "variants alternated call by call in one process; wall ms per call from pinned memory",
           "not_measured": "any 2-, 4- or 8-device figure and the RCCL branch of bv_group_verify_events "
                           "(logical shards share one GPU; group2 / group4 are recorded, not judged)",
           "variants": {}}
    for k in order:
        x = np.array(ts[k])
        out["variants"][k] = {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x.min()), 4),
                              "max_ms": round(float(x.max()), 4),
                              "events_per_s": round(n / float(np.median(x)) * 1e3),
                              "calls_ms": [round(float(v), 3) for v in x]}
        print(f"{k:9s} median {np.median(x):8.3f} ms  min {x.min():8.3f}  max {x.max():8.3f}  "
              f"{n / np.median(x) / 1e3:7.1f} M events/s", flush=True)
    base = "parent" if a.parent_lib else "verifier"
    bx = np.array(ts[base])
    half = [float(np.median(bx[i::2])) for i in (0, 1)]  # the baseline's own repeats, in this same run
    out["baseline"] = base
    out["verifier_calls_timing"] = breakdown
    out["baseline_spread_ms"] = {"half_medians": [round(h, 4) for h in half],
                                 "min_max": round(float(bx.max() - bx.min()), 4),
                                 "iqr": round(float(np.percentile(bx, 75) - np.percentile(bx, 25)), 4)}
    print("baseline", base, "spread ms", out["baseline_spread_ms"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for h in handles.values():
        h.close()
    arena.close()


if __name__ == "__main__":
    main()
