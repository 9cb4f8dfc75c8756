"""Rehearsal of bv_group_verify_blocks on one GPU (development tool): the C5
shape (tests/block_cases.synth_like_bodies: 10,000 blocks x 100 validator
signatures, 16 x 64-B transactions; valid signatures as keys.EncodeSignature
text, one in a thousand corrupted) from pinned memory through

    parent     (--parent-lib PATH) bv_verify_blocks of ANOTHER build of the
               library, the parent commit's, from its own pinned arena
    verifier   this tree's bv_verify_blocks (one context, the un-based kernel)
    group1     Group([0])           bv_group_verify_blocks (plan + gather only)
    group2     Group([0, 0])        2 logical shards
    group4     Group([0, 0, 0, 0])  4 logical shards

--variants runs a subset (e.g. `verifier` alone beside the parent library);
--parent-first creates the parent library's context and arena before this
tree's.  bv_timing medians of the two single-context variants are recorded.
The variants alternate call by call in one process (so clocks, thermals and
other tenants' load hit them alike), in an order rotated every call; ROUNDS
(3) interleaved rounds of --calls (10) timed calls after 2 untimed ones; a
round's figure is the median of its calls, a variant's the median [min, max]
of the rounds.  Every call's statuses, digests, bits and counts are checked.

Judged (DESIGN §11.10's rule): `verifier`'s median is no more than `parent`'s
median plus parent's own max - min over the rounds: the launch / finish split
costs the single-context entry nothing.  Recorded, not judged: group1's
overhead over `verifier`, and group2 / group4, whose logical shards share one
GPU and one link (no multi-device figure is measured here, nor the RCCL
branch of the gather).
Writes profiles/group_blocks_rehearsal.json (--out).  Needs a GPU."""
import argparse
import ctypes
import dataclasses
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from babble_amd import native  # noqa: E402
from babble_amd.batch import BlockBatchBuilder  # noqa: E402
from babble_amd.verifier import BlockVerifyResult, Group, PinnedArena, Verifier, _p  # noqa: E402

ROUNDS, WARMUP = 3, 2


def workload(nb, nv):
    """(PackedBlockBatch with signature text sorted by block, the corrupted items)."""
    from oracle import gosemantics as G
    from tests import block_cases as BC

    bodies = BC.synth_like_bodies(nb)
    vs = BC.validators(nv)
    pool = BC._nonce_pool()
    kb = BlockBatchBuilder()
    for b in bodies:
        kb.add_block(b)
    for _, pub in vs:
        kb.add_key(pub)
    rng = np.random.default_rng(5)
    bad = np.sort(rng.choice(nb * nv, size=max(1, nb * nv // 1000), replace=False))
    is_bad = np.zeros(nb * nv, bool)
    is_bad[bad] = True
    texts = []
    for b, body in enumerate(bodies):
        z = int.from_bytes(hashlib.sha256(body.Marshal()).digest(), "big")
        for v, (d, _) in enumerate(vs):
            r, kinv = pool[(b + v) % 4]
            s = kinv * (z + r * d) % G.N
            if is_bad[b * nv + v]:
                s = s % (G.N - 2) + 1  # another s in [1, N): REJECT
            texts.append(G.EncodeSignature(r, s).encode())
    off = np.zeros(nb * nv + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in texts])
    pb = kb.pack()
    pb = dataclasses.replace(pb, item_block=np.repeat(np.arange(nb, dtype=np.uint32), nv),
                             item_key=np.tile(np.arange(nv, dtype=np.uint32), nb), sig_off=off,
                             sig_text=np.frombuffer(b"".join(texts), np.uint8).copy())
    return pb, bad


class OtherLib:
    """bv_verify_blocks of a second build of the library beside this one (only
    symbols the parent commit already has), with its own arena: each build
    DMAs in place only from its own bv_host_alloc memory."""

    def __init__(self, path):
        P = ctypes.c_void_p
        L = self._L = ctypes.CDLL(os.path.abspath(path))
        L.bv_create.argtypes = [ctypes.POINTER(P), ctypes.c_int, ctypes.c_uint32]
        L.bv_destroy.argtypes = [P]
        L.bv_verify_blocks.argtypes = [P, ctypes.POINTER(native.BvBlockBatch), ctypes.POINTER(native.BvResult), P]
        L.bv_get_timing.argtypes = [P, ctypes.POINTER(native.BvTiming)]
        L.bv_host_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(P)]
        L.bv_host_free.argtypes = [P]
        L.bv_host_free.restype = None
        self.ctx = P()
        rc = L.bv_create(ctypes.byref(self.ctx), 0, 0)
        if rc != native.BV_OK:
            raise native.BvError(rc, "bv_create (other library)")
        self.arena = PinnedArena(lib=L)

    def call(self, cb, r, vc):
        return self._L.bv_verify_blocks(self.ctx, ctypes.byref(cb), ctypes.byref(r), vc)

    def timing(self):
        t = native.BvTiming()
        self._L.bv_get_timing(self.ctx, ctypes.byref(t))
        return {k: getattr(t, k) for k, _ in native.BvTiming._fields_}

    def close(self):
        self._L.bv_destroy(self.ctx)
        self.arena.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10_000)
    ap.add_argument("--validators", type=int, default=100)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variants", default="verifier,group1,group2,group4",
                    help="which of verifier, group1, group2, group4 to run (the full set is the rehearsal)")
    ap.add_argument("--parent-first", action="store_true",
                    help="create the parent library's context, arena and batch before this tree's (the two builds "
                         "hold separate streams and pinned arenas; which comes first is not neutral)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_blocks_rehearsal.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("group_blocks_rehearsal: no GPU")
    pb, bad = workload(a.blocks, a.validators)
    n, ni = pb.n_blocks, pb.n_items
    want = np.ones(ni, np.uint8)
    want[bad] = 0
    want_cnt = np.bincount(pb.item_block[want == 1], minlength=n).astype(np.uint32)
    want_bits = np.packbits(want, bitorder="little")
    want_bits = np.concatenate([want_bits, np.zeros(-len(want_bits) % 8, np.uint8)]).view(np.uint64)
    bodies, boff = pb.bodies()
    want_dig = np.frombuffer(b"".join(hashlib.sha256(bodies[int(boff[b]):int(boff[b + 1])]).digest() for b in range(n)),
                             np.uint8).reshape(n, 32)

    L = native.lib()
    keep = []
    other = OtherLib(a.parent_lib) if a.parent_lib and a.parent_first else None

    def prepared(ar):
        p = ar.block_batch(pb)
        res = BlockVerifyResult(ar.array((n, 32), np.uint8), ar.array(ni, np.uint8),
                                ar.array((ni + 63) // 64, np.uint64), ar.array(n, np.uint32))
        return p.c_struct(keep), native.BvResult(_p(res.msg_hash), _p(res.status), _p(res.accept_bits)), res

    # the C structs once, so that only the C calls are timed
    if other:
        ocb, ocr, ores = prepared(other.arena)
    arena = PinnedArena()
    cb, cr, res = prepared(arena)
    vc = _p(res.valid_count)
    make = {"verifier": lambda: Verifier(0), "group1": lambda: Group([0]), "group2": lambda: Group([0, 0]),
            "group4": lambda: Group([0, 0, 0, 0])}
    handles = {k: make[k]() for k in a.variants.split(",")}
    calls = {}
    for k, h in handles.items():
        if k == "verifier":
            calls[k] = lambda h=h: L.bv_verify_blocks(h._ctx, ctypes.byref(cb), ctypes.byref(cr), vc)
        else:
            calls[k] = lambda h=h: L.bv_group_verify_blocks(h._g, ctypes.byref(cb), ctypes.byref(cr), vc)
    results = {k: res for k in calls}
    if a.parent_lib:
        if not other:
            other = OtherLib(a.parent_lib)
            ocb, ocr, ores = prepared(other.arena)
        handles["parent"] = other
        calls["parent"] = lambda: other.call(ocb, ocr, _p(ores.valid_count))
        results["parent"] = ores
    order = sorted(calls)
    times = {k: [[] for _ in range(ROUNDS)] for k in order}
    phases = {k: [] for k in order if k in ("parent", "verifier")}  # bv_timing of each timed single-context call
    it = 0
    for r in range(ROUNDS):
        for c in range(WARMUP + a.calls):
            # rotated, so every variant runs equally often in every position
            for k in order[it % len(order):] + order[: it % len(order)]:
                out = results[k]
                out.status[:] = 0xEE
                out.valid_count[:] = 0xEEEEEEEE
                t0 = time.perf_counter()
                rc = calls[k]()
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == native.BV_OK, (k, rc)
                assert np.array_equal(out.status, want) and np.array_equal(out.valid_count, want_cnt), k
                assert np.array_equal(out.accept_bits, want_bits) and np.array_equal(out.msg_hash, want_dig), k
                if c >= WARMUP:
                    times[k][r].append(dt)
                    if k in phases:
                        phases[k].append(handles[k].timing())
            it += 1
    out = {"blocks": n, "items": ni, "created_first": "parent" if a.parent_first else "this tree", "rounds": ROUNDS, "warmup": WARMUP, "calls_per_round": a.calls,
           "rejections": int(len(bad)), "device": torch.cuda.get_device_name(0),
           "unit": "wall ms per call (time.perf_counter around the C call), median [min, max] of the rounds' medians",
           "method": "variants alternated call by call in one process, order rotated; pinned batch and results",
           "not_measured": "any 2- or 4-device figure and the RCCL branch of the gather (logical shards share one "
                           "GPU and one link; group2 / group4 are recorded, not judged)",
           "variants": {}}
    for k in order:
        med = [statistics.median(x) for x in times[k]]
        out["variants"][k] = {"median_ms": round(statistics.median(med), 4), "min_ms": round(min(med), 4),
                              "max_ms": round(max(med), 4), "rounds_ms": [round(m, 4) for m in med],
                              "calls_ms": [[round(v, 3) for v in x] for x in times[k]]}
        print(f"{k:9s} median {statistics.median(med):8.3f} ms  [{min(med):8.3f}, {max(med):8.3f}]", flush=True)
    fields = ("ms_total", "ms_h2d", "ms_host_prep", "ms_sha256", "ms_keyprep", "ms_verify_g", "ms_verify", "ms_d2h",
              "ms_host", "ms_host_out")
    out["bv_timing_median"] = {k: {f: round(statistics.median(t[f] for t in ts), 4) for f in fields}
                               for k, ts in phases.items()}
    for k, t in out["bv_timing_median"].items():
        print(f"{k:9s} bv_timing medians {t}", flush=True)
    v = out["variants"]
    if "group1" in v and "verifier" in v:
        out["recorded"] = {"group1_minus_verifier_ms": round(v["group1"]["median_ms"] - v["verifier"]["median_ms"], 4)}
    if a.parent_lib and "verifier" in v:
        p = v["parent"]
        out["judged"] = {"rule": "verifier median <= parent median + (parent max - min over the rounds)",
                         "parent_spread_ms": round(p["max_ms"] - p["min_ms"], 4),
                         "verifier_minus_parent_ms": round(v["verifier"]["median_ms"] - p["median_ms"], 4),
                         "holds": v["verifier"]["median_ms"] <= p["median_ms"] + (p["max_ms"] - p["min_ms"])}
        print("judged", out["judged"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for h in handles.values():
        h.close()
    arena.close()


if __name__ == "__main__":
    main()
