"""Same-box A/B of bv_verify_events_itx (development tool): one process, one
library, one context; the entries alternate call by call, so clock drift
hits both alike.

(a) A SyncResponse-shaped batch: 1000 events of 4 creators in ~333 in-batch
    levels, with 0, 10 and 1000 InternalTransactions, every signature valid,
    every input and result array in bv_host_alloc memory.
      new    ONE bv_verify_events_itx call over the fields
      today  bv_verify_events over the ITX JSON fragments, then bv_verify_batch
             over the ITX items, plus the host work that feeds them, timed on
             its own: both JSON forms of every ITX (the list element and
             Body.Marshal()), bv_hex_decode and bv_decode_signature per ITX.
             That host work is this package's Python mirror (babble_amd/
             gojson.py), NOT Go's encoding/json: its share is an upper bound of
             what a Go caller saves.
(b) 1M bulk events (every parent a known hash) without ITXs through the new
    entry (all lists nil) against bv_verify_events over the same events with
    signature text, alternated; `inside_spread`: the new entry's median lies
    inside [min, max] of bv_verify_events' round medians.

Per shape ROUNDS (3) rounds of `--calls` alternated calls after 2 untimed
ones; a round's figure is the median of its calls, a shape's the median
[min, max] of the rounds.

  python tools/ab_event_itx.py [--out profiles/event_itx_ab.json] [--calls 10] [--bulk 1000000]
"""
import argparse
import ctypes
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
from babble_amd.batch import BatchBuilder  # noqa: E402
from babble_amd.verifier import PinnedArena, Verifier, VerifyResult, _cbatch, _p  # noqa: E402

ROUNDS, WARMUP = 3, 2


def rounds_stat(per_round):
    med = [statistics.median(r) for r in per_round]
    return {"median": statistics.median(med), "min": min(med), "max": max(med), "rounds": med}


def sync_case(n_itx, n=1000):
    from tests import itx_cases as C

    every = n // n_itx if n_itx else 0
    specs = []
    for e in range(n):
        par = [("event", e - 4) if e >= 4 else None, ("event", e - 3) if e >= 3 else None]
        itxs = [C.make_itx(e % 4, typ=e % 2, netaddr="node%d.example:1337" % e, moniker="node%d" % e)] \
            if every and e % every == 0 else None
        specs.append(dict(c=e % 4, index=e // 4, ts=1600000000 + e, parents=par, txs=[bytes([e % 251]) * 64], itxs=itxs))
    return C.ItxCase(specs), specs


def mirror(t):
    return H.InternalTransaction(H.InternalTransactionBody(t.Body.Type, H.Peer(t.Body.Peer.NetAddr, t.Body.Peer.PubKeyHex,
                                                                             t.Body.Peer.Moniker)), t.Signature)


def run_sync(v, n_itx, calls):
    from tests import itx_cases as C

    c, specs = sync_case(n_itx)
    n, m = c.n, c.packed.n_itx
    assert m == n_itx
    itxs = [[mirror(t) for t in (b.InternalTransactions or [])] for b in c.bodies]
    flat = [t for l in itxs for t in l]

    def host_work():
        """today's host side: both JSON forms, key and signature decode per ITX"""
        frags = [b"" if not l else b"[" + b",".join(t.json() for t in l) + b"]" for l in itxs]
        msgs = [t.Body.Marshal() for t in flat]
        keys = [native.hex_decode(t.Body.Peer.PubKeyHex) for t in flat]
        sigs = [native.decode_signature(t.Signature) for t in flat]
        return frags, msgs, keys, sigs

    frags, msgs, keys, sigs = host_work()
    fb = E.EventBatchBuilder()
    for k in range(4):
        fb.add_key(C.validators(4)[k][1])
    for s, b, sig, fr in zip(specs, c.bodies, c.signatures, frags):
        fb.add_event(s["c"], b.Index, b.Timestamp, s["parents"], b.Transactions, sig,
                     itx_json=b"" if b.InternalTransactions is None else fr)
    wire = fb.pack()
    so = np.zeros(n + 1, np.uint64)
    so[1:] = np.cumsum([len(x) for x in c.signatures])
    wire = wire.with_signature_text(np.frombuffer("".join(c.signatures).encode(), np.uint8).copy(), so)
    bb = BatchBuilder()
    for msg, key, (pre, r, s) in zip(msgs, keys, sigs):
        bb.add_item_raw(bb.add_msg(msg), bb.add_key(key), pre, r, s)
    arena = PinnedArena()
    L = native.lib()
    keep = []
    xp, wp = arena.event_itx_batch(c.packed), arena.wire(wire)
    cx, cw = xp.c_struct(keep), wp.c_struct(keep)
    cbat = _cbatch(arena.batch(bb.pack()), keep) if m else None
    rn = VerifyResult(arena.array((n, 32), np.uint8), arena.array(n, np.uint8), arena.array((n + 63) // 64, np.uint64))
    rt = VerifyResult(arena.array((n, 32), np.uint8), arena.array(n, np.uint8), arena.array((n + 63) // 64, np.uint64))
    ri = VerifyResult(arena.array((max(m, 1), 32), np.uint8), arena.array(max(m, 1), np.uint8),
                      arena.array((m + 63) // 64 + 1, np.uint64))
    ih, ist, by = arena.array((max(m, 1), 32), np.uint8), arena.array(max(m, 1), np.uint8), arena.array(n, np.uint32)
    crn = native.BvResult(_p(rn.msg_hash), _p(rn.status), _p(rn.accept_bits))
    crt = native.BvResult(_p(rt.msg_hash), _p(rt.status), _p(rt.accept_bits))
    cri = native.BvResult(_p(ri.msg_hash), _p(ri.status), _p(ri.accept_bits))
    cout = E.BvEventItxOut(_p(ih), _p(ist), _p(by))

    def new_call():
        assert L.bv_verify_events_itx(v._ctx, ctypes.byref(cx), ctypes.byref(crn), ctypes.byref(cout)) == native.BV_OK

    def today_calls():
        assert L.bv_verify_events(v._ctx, ctypes.byref(cw), ctypes.byref(crt)) == native.BV_OK
        if m:
            assert L.bv_verify_batch(v._ctx, ctypes.byref(cbat), ctypes.byref(cri)) == native.BV_OK

    times = {k: [[] for _ in range(ROUNDS)] for k in ("new", "today_calls", "today_host")}
    for r in range(ROUNDS):
        for k in range(WARMUP + calls):
            for name, fn in (("new", new_call), ("today_calls", today_calls), ("today_host", host_work)):
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if k >= WARMUP:
                    times[name][r].append(dt)
            assert (rn.status == 1).all() and (rt.status == 1).all() and np.array_equal(rn.msg_hash, rt.msg_hash)
            assert (ist[:m] == 1).all() and (ri.status[:m] == 1).all() and np.array_equal(ih[:m], ri.msg_hash[:m])
    t_new = v_timing(v, new_call)
    st = {k: rounds_stat(x) for k, x in times.items()}
    today = st["today_calls"]["median"] + st["today_host"]["median"]
    cell = {"events": n, "itxs": m, "call_ms": st, "today_total_ms": today,
            "today_host_share": st["today_host"]["median"] / today if today else 0.0,
            "new_small_path": t_new["ms_h2d"] == 0, "new_key_path": t_new["key_path"]}
    arena.close()
    return cell


def v_timing(v, call):
    call()
    return v.timing()


def run_bulk(v, n, calls):
    from tests.cabi import harness

    _, wire = synth.event_fields(n, n_creators=64, seed=2, parents="hash")
    text, off = harness.encode_signatures(wire.r_be, wire.s_be)
    wire = wire.with_signature_text(np.asarray(text, np.uint8), np.asarray(off, np.uint64))
    xb = E.PackedEventItxBatch(events=wire, itx_start=np.zeros(n + 1, np.uint64), itx_list_nil=np.ones(n, np.uint8),
                               itx_type=np.zeros(0, np.uint8), itx_str_off=np.zeros(1, np.uint64),
                               itx_str=np.zeros(0, np.uint8))
    arena = PinnedArena()
    L = native.lib()
    keep = []
    xp = arena.event_itx_batch(xb)
    cx, cw = xp.c_struct(keep), xp.events.c_struct(keep)
    res = {k: VerifyResult(arena.array((n, 32), np.uint8), arena.array(n, np.uint8), arena.array((n + 63) // 64, np.uint64))
           for k in ("events", "events_itx")}
    cres = {k: native.BvResult(_p(r.msg_hash), _p(r.status), _p(r.accept_bits)) for k, r in res.items()}
    by = arena.array(n, np.uint32)
    cout = E.BvEventItxOut(None, None, _p(by))
    res["events_itx_no_out"] = res["events_itx"]  # (the same call without decided_by: what that 4 MB write costs)
    cres["events_itx_no_out"] = cres["events_itx"]
    fns = {"events": lambda: L.bv_verify_events(v._ctx, ctypes.byref(cw), ctypes.byref(cres["events"])),
           "events_itx_no_out": lambda: L.bv_verify_events_itx(v._ctx, ctypes.byref(cx),
                                                               ctypes.byref(cres["events_itx"]), None),
           "events_itx": lambda: L.bv_verify_events_itx(v._ctx, ctypes.byref(cx), ctypes.byref(cres["events_itx"]),
                                                        ctypes.byref(cout))}
    times = {k: [[] for _ in range(ROUNDS)] for k in fns}
    for r in range(ROUNDS):
        for k in range(WARMUP + calls):
            for name, fn in fns.items():
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == native.BV_OK and (res[name].status == 1).all(), name
                if k >= WARMUP:
                    times[name][r].append(dt)
    assert np.array_equal(res["events"].msg_hash, res["events_itx"].msg_hash) and (by == E.EV_SELF).all()
    st = {k: rounds_stat(x) for k, x in times.items()}
    a, b = st["events"], st["events_itx"]
    cell = {"events": n, "call_ms": st, "events_spread_ms": a["max"] - a["min"],
            "itx_minus_events_ms": b["median"] - a["median"], "inside_spread": a["min"] <= b["median"] <= a["max"],
            "no_slower_than_events_max": b["median"] <= a["max"]}
    arena.close()
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_itx_ab.json"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--bulk", type=int, default=1_000_000)
    a = ap.parse_args()
    out = {"unit": "wall ms per call (time.perf_counter around the C calls), median [min, max] of 3 interleaved rounds' "
                   "medians", "rounds": ROUNDS, "warmup": WARMUP, "calls_per_round": a.calls,
           "host_note": "today_host is this package's Python mirror (gojson.py) and ctypes calls, not Go",
           "sync_1000_events": {}, "bulk_no_itx": None}
    v = Verifier(0)
    for k in (0, 10, 1000):
        cell = run_sync(v, k, a.calls)
        out["sync_1000_events"]["itx_%d" % k] = cell
        print("sync 1000 events, %4d ITXs: new %.3f ms; today %.3f (calls) + %.3f (host, Python) ms, host share %.2f"
              % (k, cell["call_ms"]["new"]["median"], cell["call_ms"]["today_calls"]["median"],
                 cell["call_ms"]["today_host"]["median"], cell["today_host_share"]), flush=True)
    if a.bulk:
        cell = run_bulk(v, a.bulk, a.calls)
        out["bulk_no_itx"] = cell
        print("bulk %d events, no ITXs: events %s  events_itx %s  inside spread: %s"
              % (a.bulk, cell["call_ms"]["events"], cell["call_ms"]["events_itx"], cell["inside_spread"]), flush=True)
    v.close()
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1, sort_keys=True)
        fo.write("\n")


if __name__ == "__main__":
    main()
