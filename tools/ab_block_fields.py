"""Same-box A/B of the two ways a batch of blocks reaches the device
(development tool): one process, one library, one context; the entries
alternate call by call, so clock drift hits both alike.

  text    bv_verify_batch_text over pre-serialised BlockBody.Marshal() bytes
          (the baseline: that path is what it was before bv_verify_blocks)
  fields  bv_verify_blocks over the BlockBody fields: the library builds and
          hashes the bodies (valid_count asked for, status too)

Shapes: C5 (10,000 blocks x 100 validators, 16 x 64-B transactions), one
100-item block, one ~40 KB block with 100 items; valid signatures as
keys.EncodeSignature text; every input and result array in bv_host_alloc
memory.  The fields are parsed back from the synthetic generator's bodies and
bv_block_bodies must reproduce those bodies byte for byte before anything is
timed.  Per shape ROUNDS (3) interleaved rounds of `--calls` alternated calls
after 2 untimed ones; a round's figure is the median of its calls, a shape's
the median [min, max] of the rounds.

Reported per shape: (a) the call time of each entry; (b) the bytes each entry
stages per call; (c) the host serialisation the caller of `fields` no longer
pays, timed with bv_block_bodies on one thread and on 8 threads over block
slices — the C emitter's time, NOT Go's encoding/json; bv_timing of each
entry's last call; the acceptance comparisons.  On C5 also both workgroup
sizes of k_blk_body_hash (contexts created under BV_BLK_NT=64 / 256).

  python tools/ab_block_fields.py [--out profiles/block_fields_ab.json] [--calls 10]
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
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from babble_amd import hashgraph as H  # noqa: E402
from babble_amd import native, synth  # noqa: E402
from babble_amd.batch import BlockBatchBuilder, PackedTextBatch  # noqa: E402
from babble_amd.verifier import BlockVerifyResult, PinnedArena, Verifier, VerifyResult, _ctbatch, _p  # noqa: E402

ROUNDS, WARMUP, THREADS = 3, 2, 8
# (name, blocks, validators, transactions, bytes per transaction)
SHAPES = (("c5_10000x100", 10_000, 100, 16, 64), ("block_1x100", 1, 100, 16, 64), ("block40k_1x100", 1, 100, 16, 1870))


def workload(nb, nv, n_tx, tx_bytes):
    """(PackedTextBatch over the generator's bodies, PackedBlockBatch of the same blocks' fields)."""
    from tests.cabi import harness

    b = synth.blocks(nb, nv, seed=5, n_tx=n_tx, tx_bytes=tx_bytes).batch
    text, off = harness.encode_signatures(b.r_be, b.s_be)
    off = np.asarray(off, np.uint64)
    kb = BlockBatchBuilder()

    def dec(x):
        return None if x is None else base64.b64decode(x)

    def frag(x):
        assert x is None or x == [], x  # (the generator's blocks carry no internal transactions)
        return None if x is None else b"[]"

    for m in range(nb):
        j = json.loads(b.message(m))
        kb.add_block(H.BlockBody(j["Index"], j["RoundReceived"], j["Timestamp"], dec(j["StateHash"]), dec(j["FrameHash"]),
                                 dec(j["PeersHash"]),
                                 None if j["Transactions"] is None else [dec(t) for t in j["Transactions"]],
                                 frag(j["InternalTransactions"]), frag(j["InternalTransactionReceipts"])))
    for k in range(b.n_keys):
        kb.add_key(b.key(k))
    pb = kb.pack()
    pb = dataclasses.replace(pb, item_block=b.item_msg.astype(np.uint32), item_key=b.item_key.astype(np.uint32),
                             sig_off=off, sig_text=np.asarray(text, np.uint8))
    assert np.array_equal(pb.key_bytes, b.key_bytes)
    bodies, boff = pb.bodies()
    assert np.array_equal(boff, b.msg_off) and bodies.tobytes() == b.msg_bytes.tobytes(), "fields do not give the bodies"
    tb = PackedTextBatch(b.msg_bytes, b.msg_off, b.key_bytes, b.key_off, b.item_msg, b.item_key, off,
                         np.asarray(text, np.uint8))
    return tb, pb


def block_slice(pb, a, z):
    """Blocks [a, z) of pb as a batch of their own (offsets rebased; no items)."""
    t0, t1 = int(pb.tx_start[a]), int(pb.tx_start[z])

    def cut(off, data, lo, hi):
        o = off[lo:hi + 1]
        return (o - o[0]).astype(np.uint64), data[int(o[0]):int(o[-1])].copy()

    ho, hb = cut(pb.hash_off, pb.hash_bytes, 3 * a, 3 * z)
    to, tbytes = cut(pb.tx_off, pb.tx_bytes, t0, t1)
    io, ij = (None, pb.itx_json[:0]) if pb.itx_off is None else cut(pb.itx_off, pb.itx_json, a, z)
    ro, rj = (None, pb.rcpt_json[:0]) if pb.rcpt_off is None else cut(pb.rcpt_off, pb.rcpt_json, a, z)
    return dataclasses.replace(
        pb, index=pb.index[a:z].copy(), round_received=pb.round_received[a:z].copy(),
        timestamp=pb.timestamp[a:z].copy(), hash_off=ho, hash_bytes=hb,
        hash_nil=None if pb.hash_nil is None else pb.hash_nil[3 * a:3 * z].copy(),
        tx_start=(pb.tx_start[a:z + 1] - pb.tx_start[a]).astype(np.uint64), tx_off=to, tx_bytes=tbytes,
        tx_list_nil=None if pb.tx_list_nil is None else pb.tx_list_nil[a:z].copy(),
        tx_nil=None if pb.tx_nil is None else pb.tx_nil[t0:t1].copy(), itx_off=io, itx_json=ij, rcpt_off=ro,
        rcpt_json=rj, item_block=np.zeros(0, np.uint32), item_key=np.zeros(0, np.uint32),
        sig_off=np.zeros(1, np.uint64), sig_text=np.zeros(0, np.uint8))


def rounds_stat(per_round):
    med = [statistics.median(r) for r in per_round]
    return {"median": statistics.median(med), "min": min(med), "max": max(med), "rounds": med}


def host_serialisation(pb, calls):
    """(c): bv_block_bodies over the whole batch on one thread, and over
    THREADS contiguous block slices on THREADS threads (ms per batch)."""
    L = native.lib()
    n = pb.n_blocks
    keep = []
    cb = pb.c_struct(keep)
    off = pb.body_lens()
    out = np.zeros(int(off[-1]), np.uint8)
    one = []
    for k in range(WARMUP + calls):
        t0 = time.perf_counter()
        rc = L.bv_block_bodies(cb, off.ctypes.data, out.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == native.BV_OK
        if k >= WARMUP:
            one.append(dt * 1e3)
    res = {"one_thread_ms": {"median": statistics.median(one), "min": min(one), "max": max(one)},
           "body_bytes": int(off[-1])}
    parts = min(THREADS, n)
    if parts > 1:
        cuts = [n * i // parts for i in range(parts + 1)]
        jobs = []
        for a, z in zip(cuts, cuts[1:]):
            sl = block_slice(pb, a, z)
            k2 = []
            c2 = sl.c_struct(k2)
            o2 = sl.body_lens()
            jobs.append((c2, o2, np.zeros(int(o2[-1]), np.uint8), k2))
        pool = ThreadPoolExecutor(parts)

        def run(j):
            assert L.bv_block_bodies(j[0], j[1].ctypes.data, j[2].ctypes.data) == native.BV_OK

        many = []
        for k in range(WARMUP + calls):
            t0 = time.perf_counter()
            list(pool.map(run, jobs))
            dt = time.perf_counter() - t0
            if k >= WARMUP:
                many.append(dt * 1e3)
        pool.shutdown()
        assert b"".join(j[2].tobytes() for j in jobs) == out.tobytes()
        res["threads"] = parts
        res["threads_ms"] = {"median": statistics.median(many), "min": min(many), "max": max(many)}
    return res


def run_shape(v, tb, pb, calls, extra=()):
    """One shape: `text` and `fields` (and any extra (name, verifier) running
    `fields` on another context) alternated; ROUNDS rounds."""
    arena = PinnedArena()
    tbp, pbp = arena.text_batch(tb), arena.block_batch(pb)
    n, ni = pb.n_blocks, pb.n_items
    rt = VerifyResult(arena.array((n, 32), np.uint8), arena.array(ni, np.uint8), arena.array((ni + 63) // 64, np.uint64))
    rf = BlockVerifyResult(arena.array((n, 32), np.uint8), arena.array(ni, np.uint8),
                           arena.array((ni + 63) // 64, np.uint64), arena.array(n, np.uint32))
    # the C structs once, so that only the C calls are timed
    L = native.lib()
    keep = []
    ctb, cpb = _ctbatch(tbp, keep), pbp.c_struct(keep)
    crt = native.BvResult(_p(rt.msg_hash), _p(rt.status), _p(rt.accept_bits))
    crf = native.BvResult(_p(rf.msg_hash), _p(rf.status), _p(rf.accept_bits))

    vcp = _p(rf.valid_count)

    def text_call():
        assert L.bv_verify_batch_text(v._ctx, ctypes.byref(ctb), ctypes.byref(crt)) == native.BV_OK

    def fields_call(vx):
        assert L.bv_verify_blocks(vx._ctx, ctypes.byref(cpb), ctypes.byref(crf), vcp) == native.BV_OK

    entries = [("text", text_call, v, rt), ("fields", lambda: fields_call(v), v, rf)]
    for name, vx in extra:
        entries.append((name, (lambda vx=vx: fields_call(vx)), vx, rf))
    times = {name: [[] for _ in range(ROUNDS)] for name, *_ in entries}
    sha = {name: [] for name, *_ in entries}
    timing = {}
    for r in range(ROUNDS):
        for k in range(WARMUP + calls):
            for name, fn, vx, res in entries:
                res.status[:] = 0xEE
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                assert int((res.status == native.ACCEPT).sum()) == ni, (name, np.bincount(res.status, minlength=4))
                assert np.array_equal(rf.msg_hash, rt.msg_hash) or name == "text", name
                if k >= WARMUP:
                    times[name][r].append(dt * 1e3)
                    timing[name] = vx.timing()
                    sha[name].append(timing[name]["ms_sha256"])
    assert np.array_equal(rf.valid_count, np.bincount(pb.item_block, minlength=n))
    cell = {"blocks": n, "items": ni,
            "a_call_ms": {name: rounds_stat(t) for name, t in times.items()},
            "b_staged_bytes": {"text": int(sum(np.asarray(getattr(tb, f)).nbytes for f in (
                "msg_bytes", "msg_off", "key_bytes", "key_off", "item_msg", "item_key", "sig_off", "sig_text"))),
                "fields": pb.staged_bytes()},
            "ms_sha256_median": {name: statistics.median(x) for name, x in sha.items()},
            "bv_timing_last_call": {name: {k: round(float(x), 4) for k, x in t.items()} for name, t in timing.items()},
            "small_path": {name: t["ms_h2d"] == 0 for name, t in timing.items()}}
    arena.close()
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_fields_ab.json"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    a = ap.parse_args()
    res = {"unit": "wall ms per call (time.perf_counter around the C call), median [min, max] of 3 interleaved "
                   "rounds' medians", "rounds": ROUNDS, "warmup": WARMUP, "calls_per_round": a.calls,
           "entries": {"text": "bv_verify_batch_text over pre-serialised bodies (baseline)",
                       "fields": "bv_verify_blocks over the BlockBody fields, status and valid_count returned"},
           "c_note": "host serialisation timed with bv_block_bodies: the library's C emitter, not Go's encoding/json",
           "shapes": {}}
    v = Verifier(0)
    for name, nb, nv, n_tx, tx_bytes in SHAPES:
        if a.shapes and name not in a.shapes.split(","):
            continue
        tb, pb = workload(nb, nv, n_tx, tx_bytes)
        extra = []
        if name.startswith("c5"):  # both workgroup sizes of k_blk_body_hash, each on a context of its own
            for nt in (64, 256):
                os.environ["BV_BLK_NT"] = str(nt)
                extra.append((f"fields_nt{nt}", Verifier(0)))
            del os.environ["BV_BLK_NT"]
        cell = run_shape(v, tb, pb, a.calls, extra)
        for _, vx in extra:
            vx.close()
        cell["c_host_serialisation"] = host_serialisation(pb, a.calls)
        t, f = cell["a_call_ms"]["text"], cell["a_call_ms"]["fields"]
        c1 = cell["c_host_serialisation"]["one_thread_ms"]["median"]
        cell["acceptance"] = {
            "text_spread_ms": t["max"] - t["min"],
            "fields_minus_text_ms": f["median"] - t["median"],
            "fields_no_slower_than_text_plus_spread": f["median"] <= t["median"] + (t["max"] - t["min"]),
            "fields_below_text_plus_one_thread_serialisation": f["median"] < t["median"] + c1}
        res["shapes"][name] = cell
        print(f"{name:16s} text {t['median']:.3f} [{t['min']:.3f}, {t['max']:.3f}]  fields {f['median']:.3f} "
              f"[{f['min']:.3f}, {f['max']:.3f}] ms  staged {cell['b_staged_bytes']}  serialise 1 thread "
              f"{c1:.3f} ms  sha {cell['ms_sha256_median']}  {cell['acceptance']}", flush=True)
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1, sort_keys=True)
            fo.write("\n")
    v.close()


if __name__ == "__main__":
    main()
