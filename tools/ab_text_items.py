"""Same-box A/B of the three ways an item batch's signatures reach the device
(development tool): one process, one library, one context; the variants
alternate call by call, so clock drift hits all of them alike.

  a   the shim's present sequence: one bv_decode_signature call per item
      (a C loop through a function pointer, compiled here: what cgo does
      minus cgo's own per-call cost), then bv_verify_batch.  Both parts timed.
  b   bv_decode_signatures (one call), then bv_verify_batch.  Both parts timed.
  c   bv_verify_batch_text: the text goes to the library as it is.

Shapes: C5 (10,000 blocks x 100 validators = 10^6 items), one block of 100
items, 1 item; valid signatures written by keys.EncodeSignature.  Every shape
runs with every input and result array in bv_host_alloc memory (as the shim's
arenas are); C5 also runs from pageable memory.  Per cell 2 untimed and
CALLS (>= 20) timed calls of each variant, wall clock (time.perf_counter)
around the C calls; median and min-max go to the JSON file.

  python tools/ab_text_items.py [--out profiles/text_items_ab.json] [--calls 20]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from babble_amd import native, synth  # noqa: E402
from babble_amd.verifier import PinnedArena, Verifier, _p  # noqa: E402

LOOP_C = r"""
#include <stddef.h>
#include <stdint.h>
typedef uint8_t (*decode_fn)(const char *, size_t, uint8_t *, uint8_t *);
void ab_decode_loop(decode_fn f, uint64_t n, const uint64_t *off, const uint8_t *text, uint8_t *r, uint8_t *s,
                    uint8_t *pre) {
  for (uint64_t i = 0; i < n; i++)
    pre[i] = f((const char *)text + off[i], (size_t)(off[i + 1] - off[i]), r + 32 * i, s + 32 * i);
}
"""
SHAPES = (("c5_10000x100", 10_000, 100, ("pinned", "pageable")), ("block_1x100", 1, 100, ("pinned",)),
          ("item_1x1", 1, 1, ("pinned",)))
WARMUP = 2


def decode_loop(tmp):
    src, so = os.path.join(tmp, "ab_loop.c"), os.path.join(tmp, "ab_loop.so")
    with open(src, "w") as f:
        f.write(LOOP_C)
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-o", so, src], check=True)
    L = ctypes.CDLL(so)
    P = ctypes.c_void_p
    L.ab_decode_loop.argtypes = [P, ctypes.c_uint64, P, P, P, P, P]
    L.ab_decode_loop.restype = None
    return L.ab_decode_loop


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_cell(v, loop, b, text, off, memory, calls):
    """One (shape, memory) cell: every variant `WARMUP + calls` times, alternated."""
    L = native.lib()
    arena = PinnedArena() if memory == "pinned" else None
    put = arena.copy if arena else (lambda a: np.ascontiguousarray(a).copy())
    new = (lambda shape, dt: arena.array(shape, dt)) if arena else (lambda shape, dt: np.zeros(shape, dt))
    n, nm = b.n_items, b.n_msgs
    arr = {k: put(getattr(b, k)) for k in ("msg_bytes", "msg_off", "key_bytes", "key_off", "item_msg", "item_key")}
    arr["sig_off"], arr["sig_text"] = put(off.astype(np.uint64)), put(text)
    r, s, pre = new((n, 32), np.uint8), new((n, 32), np.uint8), new(n, np.uint8)  # where a / b decode into
    h, st, bits = new((nm, 32), np.uint8), new(n, np.uint8), new((n + 63) // 64, np.uint64)
    tb = native.BvTextBatch()
    cb = tb.items
    cb.n_msgs, cb.n_keys, cb.n_items = nm, b.n_keys, n
    for k in ("msg_bytes", "msg_off", "key_bytes", "key_off", "item_msg", "item_key"):
        setattr(cb, k, _p(arr[k]))
    tb.sig_off, tb.sig_text = _p(arr["sig_off"]), _p(arr["sig_text"])
    hb = native.BvBatch()  # the same batch over the decoded arrays
    ctypes.memmove(ctypes.byref(hb), ctypes.byref(cb), ctypes.sizeof(hb))
    hb.r_be, hb.s_be, hb.pre = _p(r), _p(s), _p(pre)
    res = native.BvResult(_p(h), _p(st), _p(bits))
    one = ctypes.cast(L.bv_decode_signature, ctypes.c_void_p)
    now = time.perf_counter

    def verify():
        rc = L.bv_verify_batch(v._ctx, ctypes.byref(hb), ctypes.byref(res))
        assert rc == native.BV_OK, L.bv_last_error(v._ctx)

    def a():
        t0 = now()
        loop(one, n, _p(arr["sig_off"]), _p(arr["sig_text"]), _p(r), _p(s), _p(pre))
        t1 = now()
        verify()
        return t1 - t0, now() - t1

    def bb():
        t0 = now()
        rc = L.bv_decode_signatures(n, _p(arr["sig_off"]), _p(arr["sig_text"]), _p(r), _p(s), _p(pre))
        t1 = now()
        assert rc == native.BV_OK
        verify()
        return t1 - t0, now() - t1

    def c():
        t0 = now()
        rc = L.bv_verify_batch_text(v._ctx, ctypes.byref(tb), ctypes.byref(res))
        assert rc == native.BV_OK, L.bv_last_error(v._ctx)
        return 0.0, now() - t0

    out = {name: {"decode": [], "verify": [], "total": []} for name in "abc"}
    digests = None
    for k in range(WARMUP + calls):
        for name, fn in (("a", a), ("b", bb), ("c", c)):
            st[:] = 0xEE
            d, w = fn()
            assert int((st == native.ACCEPT).sum()) == n, (name, k, np.bincount(st, minlength=4))
            digests = h.copy() if digests is None else digests
            assert np.array_equal(h, digests), (name, k)
            if k >= WARMUP:
                out[name]["decode"].append(d * 1e3)
                out[name]["verify"].append(w * 1e3)
                out[name]["total"].append((d + w) * 1e3)
    t = v.timing()
    cell = {name: {part: stats(vals) for part, vals in parts.items()} for name, parts in out.items()}
    cell["items"], cell["text_bytes"] = n, int(off[-1])
    cell["c_small_path"], cell["c_key_path"] = t["ms_h2d"] == 0, t["key_path"]
    sa = cell["a"]["total"]
    cell["a_spread"] = sa["max"] - sa["min"]
    cell["c_minus_a"] = cell["c"]["total"]["median"] - sa["median"]
    cell["c_slower_than_a_beyond_spread"] = cell["c_minus_a"] > cell["a_spread"]
    if arena:
        arena.close()
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_items_ab.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--flags", type=int, default=native.F_DEFAULT, help="bv_create flags of the context")
    a = ap.parse_args()
    assert a.calls >= 20
    from tests.cabi import harness

    res = {"unit": "wall ms per call", "warmup": WARMUP, "calls": a.calls, "flags": a.flags,
           "variants": {"a": "bv_decode_signature per item (C loop), then bv_verify_batch",
                        "b": "bv_decode_signatures, then bv_verify_batch", "c": "bv_verify_batch_text"},
           "cells": {}}
    v = Verifier(0, flags=a.flags)
    with tempfile.TemporaryDirectory() as tmp:
        loop = decode_loop(tmp)
        for name, nb, nv, memories in SHAPES:
            b = synth.blocks(nb, nv, seed=5).batch
            text, off = harness.encode_signatures(b.r_be, b.s_be)
            for memory in memories:
                cell = run_cell(v, loop, b, text, off, memory, a.calls)
                res["cells"][f"{name}_{memory}"] = cell
                print(f"{name:14s} {memory:8s} " + "  ".join(
                    f"{x}: {cell[x]['total']['median']:.3f} ms [{cell[x]['total']['min']:.3f}, "
                    f"{cell[x]['total']['max']:.3f}] (decode {cell[x]['decode']['median']:.3f})" for x in "abc") +
                    f"  c small path: {cell['c_small_path']}", flush=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1, sort_keys=True)
                    f.write("\n")
    v.close()


if __name__ == "__main__":
    main()
