"""Rehearsal of bv_group_verify_events_fields on one GPU (development tool): 1M
bulk events (every parent a known hash) with one block signature each, the
shape of tools/ab_event_fields.py, from pinned memory through

    verifier   Verifier.verify_events_fields_into (one context, the un-based kernels)
    group1     Group([0]).verify_events_fields_into           (plan + gather only)
    group2     Group([0, 0]).verify_events_fields_into        (2 logical shards)
    group4     Group([0, 0, 0, 0]).verify_events_fields_into  (4 logical shards)
    parent     (--parent-lib PATH) bv_verify_events_fields of ANOTHER build of
               the library, e.g. the parent commit's, from its own pinned arena

The variants alternate call by call in one process (so clocks, thermals and
other tenants' load hit them alike), in an order rotated every round; after a
warm-up each gets --calls timed calls (>= 20); median and min-max per variant,
every call's time, and whether `verifier`'s median lies inside the baseline's
own min-max (the parent library's when given).  --variants runs a subset:
`verifier` alone beside the parent library is the two-alone pairing (a
one-context call is slower when the library's previous call was a group call).
--parent-first creates the other library's context and arena before this
library's; --parent-lib pointing at a byte-copy of THIS tree's library is the
control (the same code in both roles: what the pairing itself can resolve).
For `verifier` and `parent` the median of every bv_timing field over the timed
calls is recorded, so a difference can be placed on the host or on the device
timeline.
The event signatures are over the bodies WITHOUT block signatures, so every
status is REJECT in every variant (a rejected signature costs the verify
kernels what a valid one does); every variant's last result is compared with
the first's, digest by digest.  Logical shards share one GPU: group2 / group4
rehearse the multi-device code path and are recorded, not expected to be
faster; no multi-device figure is measured here.
Writes profiles/group_event_fields_rehearsal.json (--out).  Needs a GPU."""
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

from babble_amd import events as E  # noqa: E402
from babble_amd import native, synth  # noqa: E402
from babble_amd.verifier import EventItxVerifyResult, Group, PinnedArena, Verifier, _event_itx_call  # noqa: E402


class OtherLib:
    """bv_verify_events_fields of a second build of the library beside this
    one (only the symbols the parent commit already has), with its own arena:
    each build DMAs in place only from its own bv_host_alloc memory."""

    def __init__(self, path):
        P = ctypes.c_void_p
        L = self._L = ctypes.CDLL(os.path.abspath(path))
        L.bv_create.argtypes = [ctypes.POINTER(P), ctypes.c_int, ctypes.c_uint32]
        L.bv_destroy.argtypes = [P]
        L.bv_last_error.argtypes = [P]
        L.bv_last_error.restype = ctypes.c_char_p
        L.bv_verify_events_fields.argtypes = [P, P, ctypes.POINTER(native.BvResult), P]
        L.bv_host_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(P)]
        L.bv_host_free.argtypes = [P]
        L.bv_host_free.restype = None
        self.ctx = P()
        rc = L.bv_create(ctypes.byref(self.ctx), 0, 0)
        if rc != native.BV_OK:
            raise native.BvError(rc, "bv_create (other library)")
        L.bv_get_timing.argtypes = [P, ctypes.POINTER(native.BvTiming)]
        self.arena = PinnedArena(lib=L)

    def verify_events_fields_into(self, fb, res):
        rc = _event_itx_call(self._L.bv_verify_events_fields, self.ctx, fb, res)
        if rc != native.BV_OK:
            raise native.BvError(rc, self._L.bv_last_error(self.ctx).decode(errors="replace"))
        return res

    def timing(self):
        t = native.BvTiming()
        self._L.bv_get_timing(self.ctx, ctypes.byref(t))
        return {k: getattr(t, k) for k, _ in native.BvTiming._fields_}

    def close(self):
        self._L.bv_destroy(self.ctx)
        self.arena.close()


def workload(n):
    """n bulk events, one block signature each: Index = the event's, Signature
    = the event's own r|s text (~100 characters); no ITX fields."""
    from tests.cabi import harness

    _, wire = synth.event_fields(n, n_creators=64, seed=2, parents="hash")
    text, off = harness.encode_signatures(wire.r_be, wire.s_be)
    text, off = np.asarray(text, np.uint8), np.asarray(off, np.uint64)
    ev = E.PackedEventItxBatch(events=wire.with_signature_text(text, off), itx_start=None, itx_list_nil=None,
                               itx_type=np.zeros(0, np.uint8), itx_str_off=None, itx_str=np.zeros(0, np.uint8))
    return E.PackedEventFieldsBatch(ev=ev, bsig_start=np.arange(n + 1, dtype=np.uint64), bsig_list_nil=None,
                                    bsig_index=wire.index.astype(np.int64), bsig_sig_off=off.copy(), bsig_sig=text.copy(),
                                    bsig_val_kind=None, bsig_val_off=None, bsig_val_bytes=np.zeros(0, np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variants", default="verifier,group1,group2,group4",
                    help="which of verifier, group1, group2, group4 to run (the full set is the rehearsal)")
    ap.add_argument("--parent-first", action="store_true",
                    help="create the other library's context and arena before this library's (default: after)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_event_fields_rehearsal.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("group_event_fields_rehearsal: no GPU")
    if a.calls < 20:
        sys.exit("group_event_fields_rehearsal: at least 20 timed calls per variant")
    n = a.events
    fb = workload(n)

    def results(ar):
        return EventItxVerifyResult(ar.array((n, 32), np.uint8), ar.array(n, np.uint8),
                                    ar.array((n + 63) // 64, np.uint64), None, None, ar.array(n, np.uint32))

    other = OtherLib(a.parent_lib) if a.parent_lib and a.parent_first else None
    arena = PinnedArena()
    pf = arena.event_fields_batch(fb)
    make = {"verifier": lambda: Verifier(0), "group1": lambda: Group([0]), "group2": lambda: Group([0, 0]),
            "group4": lambda: Group([0, 0, 0, 0])}
    handles = {k: make[k]() for k in a.variants.split(",")}
    variants = {k: (h, pf, results(arena)) for k, h in handles.items()}
    if a.parent_lib:
        other = handles["parent"] = other or OtherLib(a.parent_lib)
        variants["parent"] = (other, other.arena.event_fields_batch(fb), results(other.arena))
    order = sorted(variants)
    ts = {k: [] for k in order}
    phases = {k: [] for k in order if k in ("verifier", "parent")}  # bv_timing of each timed single-context call
    for it in range(a.warmup + a.calls):
        # the round's order is rotated, so every variant runs equally often in
        # every position (after every other variant)
        for k in order[it % len(order):] + order[: it % len(order)]:
            h, w, r = variants[k]
            t0 = time.perf_counter()
            h.verify_events_fields_into(w, r)
            dt = (time.perf_counter() - t0) * 1e3
            if it >= a.warmup:
                ts[k].append(dt)
                if k in phases:
                    phases[k].append(h.timing())
    ref = variants[order[0]][2]
    for k in order:  # the last result of each variant against the first's
        r = variants[k][2]
        assert np.array_equal(r.msg_hash, ref.msg_hash) and r.msg_hash.any(), k
        assert np.array_equal(r.status, ref.status) and np.array_equal(r.accept_bits, ref.accept_bits), k
        assert (r.decided_by == E.EV_SELF).all(), k
    out = {"events": n, "block_signatures": fb.n_bsig, "calls": a.calls, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "method": "variants alternated call by call in one process; wall ms per call from pinned memory",
           "note": "event signatures are over the bodies without block signatures: every status is REJECT in every "
                   "variant",
           "not_measured": "any 2-, 4- or 8-device figure and the RCCL branch of gather_and_finish with this entry "
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
    for k, rows in phases.items():  # the median of every bv_timing field over the variant's timed calls
        out["variants"][k]["bv_timing_median"] = {
            f: round(float(np.median([r[f] for r in rows])), 4) for f in rows[0] if f.startswith("ms_")}
        print(k, "bv_timing medians", out["variants"][k]["bv_timing_median"], flush=True)
    out["created_first"] = "parent" if other is not None and a.parent_first else "this library"
    base = "parent" if a.parent_lib else "verifier"
    bx = np.array(ts[base])
    out["baseline"] = base
    out["baseline_min_max_ms"] = [round(float(bx.min()), 4), round(float(bx.max()), 4)]
    if "verifier" in ts:
        med = float(np.median(ts["verifier"]))
        out["verifier_median_inside_baseline_min_max"] = bool(bx.min() <= med <= bx.max())
        print("verifier median", round(med, 3), "inside", base, "min-max", out["baseline_min_max_ms"], ":",
              out["verifier_median_inside_baseline_min_max"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for h in handles.values():
        h.close()
    arena.close()


if __name__ == "__main__":
    main()
