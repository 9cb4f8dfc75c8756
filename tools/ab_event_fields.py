"""Same-box A/B of bv_verify_events_fields (development tool): one process, one
library, one context; the entries alternate call by call, so clock drift
hits both alike.  Every input and result array is in bv_host_alloc memory.

(a) A SyncResponse-shaped batch: 1000 events of 4 creators in ~333 in-batch
    levels with 0, 1 and 4 block signatures per event, every signature valid.
      new    ONE bv_verify_events_fields call over the fields (no ITX fields)
      today  bv_verify_events over pre-built BlockSignatures fragments, and,
             timed on its own, the host work that builds those fragments.
(b) 1M bulk events (every parent a known hash) with 0 and with 1 block
    signature per event, the same two entries.  `inside_spread` (0
    signatures): the new entry's median lies inside [min, max] of
    bv_verify_events' round medians.

The fragment builders are STAND-INS, not Go's encoding/json:
  host_python   this package's Python mirror (BlockSignature.json per element)
  host_c_1thr   one thread of this library's C emitter: bv_event_fields_bodies
                over the batch minus the same over the batch with its block
                signatures taken out (the emitter writes whole bodies; the
                difference is the BlockSignatures text)
For the 1M shapes the Python mirror is timed over the first 20000 events and
scaled.

Per shape ROUNDS (3) rounds of `--calls` alternated calls after 2 untimed
ones; a round's figure is the median of its calls, a shape's the median
[min, max] of the rounds.  bytes_staged: the bytes of the arrays each entry
reads (what its bulk path copies to the device; the DAG path ships digests
instead of the event fields).

  python tools/ab_event_fields.py [--out profiles/event_fields_ab.json] [--calls 10] [--bulk 1000000]
"""
import argparse
import base64
import ctypes
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from babble_amd import events as E  # noqa: E402
from babble_amd import hashgraph as H  # noqa: E402
from babble_amd import native, synth  # noqa: E402
from babble_amd.verifier import PinnedArena, Verifier, VerifyResult, _p  # noqa: E402

ROUNDS, WARMUP = 3, 2


def rounds_stat(per_round):
    med = [statistics.median(r) for r in per_round]
    return {"median": statistics.median(med), "min": min(med), "max": max(med), "rounds": med}


def nbytes(*objs):
    """Bytes of every array of the given dataclasses (EventWireBatch without
    the r / s / pre arrays a text batch does not send)."""
    total = 0
    for o in objs:
        for f in dataclasses.fields(o):
            a = getattr(o, f.name)
            if isinstance(a, np.ndarray) and f.name not in ("r_be", "s_be", "pre"):
                total += a.nbytes
    return total


def time_host(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def alternate(fns, calls, check):
    times = {k: [[] for _ in range(ROUNDS)] for k in fns}
    for r in range(ROUNDS):
        for k in range(WARMUP + calls):
            for name, fn in fns.items():
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == native.BV_OK, name
                if k >= WARMUP:
                    times[name][r].append(dt)
            check()
    return {k: rounds_stat(x) for k, x in times.items()}


def c_emit_ms(fb):
    """One thread of the library's emitter over the batch, and over the same
    batch without block signatures."""
    bare = dataclasses.replace(fb, bsig_start=np.zeros_like(fb.bsig_start), bsig_list_nil=np.ones(fb.n_events, np.uint8),
                               bsig_index=np.zeros(0, np.int64), bsig_sig_off=np.zeros(1, np.uint64),
                               bsig_sig=np.zeros(0, np.uint8), bsig_val_kind=None, bsig_val_off=None)
    L = native.lib()
    out = {}
    for name, b in (("with", fb), ("without", bare)):
        keep = []
        cb = b.c_struct(keep)
        off = np.zeros(b.n_events + 1, np.uint64)
        assert L.bv_event_fields_body_lens(ctypes.byref(cb), off.ctypes.data) == native.BV_OK
        buf = np.zeros(int(off[-1]) + 64, np.uint8)
        out[name] = time_host(lambda: L.bv_event_fields_bodies(ctypes.byref(cb), off.ctypes.data, buf.ctypes.data))
    return out


def run_pair(v, fb, wire_frag, calls, all_valid=True, host_passes=False):
    """fb: PackedEventFieldsBatch; wire_frag: the EventWireBatch (signature
    text) with the same block signatures as bsig_json fragments."""
    n = fb.n_events
    arena = PinnedArena()
    L = native.lib()
    keep = []
    fp, wp = arena.event_fields_batch(fb), arena.wire(wire_frag)
    cf, cw = fp.c_struct(keep), wp.c_struct(keep)
    res = {k: VerifyResult(arena.array((n, 32), np.uint8), arena.array(n, np.uint8), arena.array((n + 63) // 64, np.uint64))
           for k in ("new", "today")}
    cres = {k: native.BvResult(_p(r.msg_hash), _p(r.status), _p(r.accept_bits)) for k, r in res.items()}
    by = arena.array(n, np.uint32)
    cout = E.BvEventItxOut(None, None, _p(by))
    fns = {"new": lambda: L.bv_verify_events_fields(v._ctx, ctypes.byref(cf), ctypes.byref(cres["new"]), ctypes.byref(cout)),
           "today": lambda: L.bv_verify_events(v._ctx, ctypes.byref(cw), ctypes.byref(cres["today"]))}
    if host_passes:  # the 0-signature delegation taken apart: without the decided_by output, and the scans alone
        fns["new_no_out"] = lambda: L.bv_verify_events_fields(v._ctx, ctypes.byref(cf), ctypes.byref(cres["new"]), None)

    def check():
        assert np.array_equal(res["new"].msg_hash, res["today"].msg_hash)
        assert np.array_equal(res["new"].status, res["today"].status) and (by == E.EV_SELF).all()
        assert not all_valid or (res["new"].status == 1).all()

    st = alternate(fns, calls, check)
    timing = {}
    for name, fn in fns.items():
        fn()
        t = v.timing()
        timing[name] = {"ms_h2d": t["ms_h2d"], "key_path": t.get("key_path")}
    cell = {"events": n, "block_signatures": fb.n_bsig, "call_ms": st, "timing": timing,
            "bytes_staged": {"new": nbytes(fb, fb.ev, fb.ev.events), "today": nbytes(wire_frag)},
            "new_minus_today_ms": st["new"]["median"] - st["today"]["median"],
            "today_spread_ms": st["today"]["max"] - st["today"]["min"],
            "inside_spread": st["today"]["min"] <= st["new"]["median"] <= st["today"]["max"]}
    if host_passes:
        # the host passes in front of the delegation, each alone over the same pinned arrays (numpy stand-ins
        # for the library's loops: a monotone scan of bsig_start, a scan of bsig_list_nil, a 4-byte fill)
        bs, bl = fp.bsig_start, fp.bsig_list_nil
        cell["host_pass_ms"] = {
            "decided_by_fill (new - new_no_out)": st["new"]["median"] - st["new_no_out"]["median"],
            "rest (new_no_out - today)": st["new_no_out"]["median"] - st["today"]["median"],
            "numpy_monotone_scan_bsig_start": time_host(lambda: bool((bs[1:] >= bs[:-1]).all())),
            "numpy_scan_bsig_list_nil": time_host(lambda: bool(bl.all())) if bl is not None else 0.0,
            "numpy_fill_decided_by": time_host(lambda: by.fill(0xFFFFFFFF))}
    arena.close()
    return cell


def sync_case(per_event, n=1000):
    from tests import fields_cases as C

    specs, k = [], 0
    for e in range(n):
        par = [("event", e - 4) if e >= 4 else None, ("event", e - 3) if e >= 3 else None]
        bsigs = None
        if per_event:
            bsigs = [C.block_sig(e % 4, k + j, e // 4 + j) for j in range(per_event)]
            k += per_event
        specs.append(dict(c=e % 4, index=e // 4, ts=1600000000 + e, parents=par, txs=[bytes([e % 251]) * 64], bsigs=bsigs))
    return C.FieldsCase(specs, itx_fields=False)


def run_sync(v, per_event, calls):
    c = sync_case(per_event)
    mirror = [None if b.BlockSignatures is None else [H.BlockSignature(t.Validator, t.Index, t.Signature)
                                                      for t in b.BlockSignatures] for b in c.bodies]

    def host_python():
        return [b"" if l is None else b"[" + b",".join(t.json() for t in l) + b"]" for l in mirror]

    cell = run_pair(v, c.packed, c.packed_frag.events, calls)
    emit = c_emit_ms(c.packed)
    cell["fragment_build_ms"] = {"host_python": time_host(host_python), "host_c_1thr": emit["with"] - emit["without"],
                                 "c_emit_bodies_ms": emit}
    return cell


def run_bulk(v, n, per_event, calls):
    from tests.cabi import harness

    _, wire = synth.event_fields(n, n_creators=64, seed=2, parents="hash")
    text, off = harness.encode_signatures(wire.r_be, wire.s_be)
    text, off = np.asarray(text, np.uint8), np.asarray(off, np.uint64)
    wire = wire.with_signature_text(text, off)
    ev = E.PackedEventItxBatch(events=wire, itx_start=None, itx_list_nil=None, itx_type=np.zeros(0, np.uint8),
                               itx_str_off=None, itx_str=np.zeros(0, np.uint8))
    if per_event == 0:
        fb = E.PackedEventFieldsBatch(ev=ev, bsig_start=np.zeros(n + 1, np.uint64), bsig_list_nil=np.ones(n, np.uint8),
                                      bsig_index=np.zeros(0, np.int64), bsig_sig_off=np.zeros(1, np.uint64),
                                      bsig_sig=np.zeros(0, np.uint8), bsig_val_kind=None, bsig_val_off=None,
                                      bsig_val_bytes=np.zeros(0, np.uint8))
        return run_pair(v, fb, wire, calls, host_passes=True)
    # one block signature per event: Index = the event's, Signature = the event's own r|s text (~100 characters)
    index = wire.index.astype(np.int64)
    fb = E.PackedEventFieldsBatch(ev=ev, bsig_start=np.arange(n + 1, dtype=np.uint64), bsig_list_nil=None,
                                  bsig_index=index, bsig_sig_off=off.copy(), bsig_sig=text.copy(), bsig_val_kind=None,
                                  bsig_val_off=None, bsig_val_bytes=np.zeros(0, np.uint8))
    raw = text.tobytes()
    kb = wire.key_bytes.tobytes()
    b64 = [base64.b64encode(kb[int(wire.key_off[k]):int(wire.key_off[k + 1])]) for k in range(len(wire.key_off) - 1)]
    creator = wire.creator.tolist()

    def frag(e):
        return b'[{"Validator":"%s","Index":%d,"Signature":"%s"}]' % (b64[creator[e]], index[e],
                                                                     raw[int(off[e]):int(off[e + 1])])

    frags = [frag(e) for e in range(n)]
    boff = np.zeros(n + 1, np.uint64)
    boff[1:] = np.cumsum([len(x) for x in frags], dtype=np.uint64)
    wire_frag = dataclasses.replace(wire, bsig_off=boff, bsig_json=np.frombuffer(b"".join(frags), np.uint8).copy())
    # (the synthetic event signatures are over the bodies WITHOUT block signatures: every event is REJECT here,
    # in both entries; a rejected signature costs the verify kernels what a valid one does)
    cell = run_pair(v, fb, wire_frag, calls, all_valid=False)
    cell["note"] = "event signatures are over the bodies without block signatures: every status is REJECT in both entries"
    sub = min(n, 20000)
    mirror = [[H.BlockSignature(kb[int(wire.key_off[creator[e]]):int(wire.key_off[creator[e] + 1])], int(index[e]),
                                raw[int(off[e]):int(off[e + 1])].decode())] for e in range(sub)]
    py = time_host(lambda: [b"[" + b",".join(t.json() for t in l) + b"]" for l in mirror]) * (n / sub)
    emit = c_emit_ms(fb)
    cell["fragment_build_ms"] = {"host_python_scaled_from_%d" % sub: py, "host_c_1thr": emit["with"] - emit["without"],
                                 "c_emit_bodies_ms": emit}
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_fields_ab.json"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--bulk", type=int, default=1_000_000)
    a = ap.parse_args()
    out = {"unit": "wall ms per call (time.perf_counter around the C calls), median [min, max] of 3 interleaved rounds' "
                   "medians", "rounds": ROUNDS, "warmup": WARMUP, "calls_per_round": a.calls,
           "host_note": "fragment_build_ms are stand-ins (this package's Python mirror; one thread of this library's C "
                        "emitter), not Go's encoding/json",
           "sync_1000_events": {}, "bulk": {}}
    v = Verifier(0)
    for k in (0, 1, 4):
        cell = run_sync(v, k, a.calls)
        out["sync_1000_events"]["bsig_%d" % k] = cell
        print("sync 1000 events, %d block signatures each: new %.3f ms, today %.3f ms (+ fragments: %s)"
              % (k, cell["call_ms"]["new"]["median"], cell["call_ms"]["today"]["median"],
                 {x: round(y, 3) for x, y in cell["fragment_build_ms"].items() if not isinstance(y, dict)}), flush=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1, sort_keys=True)
    if a.bulk:
        for k in (0, 1):
            cell = run_bulk(v, a.bulk, k, a.calls)
            out["bulk"]["bsig_%d" % k] = cell
            print("bulk %d events, %d block signatures each: new %s  today %s  h2d %s  bytes %s  inside spread: %s"
                  % (a.bulk, k, cell["call_ms"]["new"], cell["call_ms"]["today"], cell["timing"], cell["bytes_staged"],
                     cell["inside_spread"]), flush=True)
            with open(a.out, "w") as fo:
                json.dump(out, fo, indent=1, sort_keys=True)
                fo.write("\n")
    v.close()
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1, sort_keys=True)
        fo.write("\n")


if __name__ == "__main__":
    main()
