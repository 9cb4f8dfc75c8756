"""ctypes wrapper of tests/emu_shards/_build/libbvemushards.so: the rebased
event serialiser (evjson.h evj_emit with EvjBases, what k_ev_body_hash_rb
runs per lane) on the host.  Test infrastructure only."""
from __future__ import annotations

import ctypes
import dataclasses
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_build", "libbvemushards.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
        L = ctypes.CDLL(LIB)
        L.emus_body_hash.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_void_p]
        L.emus_body_hash.restype = None
        _lib = L
    return _lib


def slice_wire(eb, a: int, z: int, hash_lo: int, hash_hi: int):
    """What shard [a, z) of `eb` ships (bv_group_verify_events): COPIES of
    its slices, the values in them unchanged, and the bases (ev, tx, txb,
    itx, bsig, ph).  The keys stay whole."""
    t0, t1 = int(eb.tx_start[a]), int(eb.tx_start[z])
    has_tx = len(eb.tx_off) > 1
    b0, b1 = (int(eb.tx_off[t0]), int(eb.tx_off[t1])) if has_tx else (0, 0)

    def frag(off, data):
        if off is None:
            return None, data[:0].copy(), 0
        lo, hi = int(off[a]), int(off[z])
        return off[a:z + 1].copy(), data[lo:hi].copy(), lo

    itx_off, itx_json, itx_base = frag(eb.itx_off, eb.itx_json)
    bsig_off, bsig_json, bsig_base = frag(eb.bsig_off, eb.bsig_json)
    sl = dataclasses.replace(
        eb, creator=eb.creator[a:z].copy(), index=eb.index[a:z].copy(), timestamp=eb.timestamp[a:z].copy(),
        parent_kind=eb.parent_kind[a:z].copy(), parent_ref=eb.parent_ref[a:z].copy(),
        parent_hashes=eb.parent_hashes[hash_lo:hash_hi].copy(), tx_start=eb.tx_start[a:z + 1].copy(),
        tx_off=eb.tx_off[t0:t1 + 1].copy() if has_tx else eb.tx_off[:0].copy(), tx_bytes=eb.tx_bytes[b0:b1].copy(),
        tx_list_nil=None if eb.tx_list_nil is None else eb.tx_list_nil[a:z].copy(),
        tx_nil=None if eb.tx_nil is None else eb.tx_nil[t0:t1].copy(),
        itx_off=itx_off, itx_json=itx_json, bsig_off=bsig_off, bsig_json=bsig_json,
        r_be=eb.r_be[a:z].copy(), s_be=eb.s_be[a:z].copy(), pre=None if eb.pre is None else eb.pre[a:z].copy())
    return sl, np.array([a, t0, b0, itx_base, bsig_base, hash_lo], np.uint64)


def body_hash(sl, bases: np.ndarray, a: int, z: int) -> np.ndarray:
    """Digests [z - a, 32] of events [a, z) from the shard's slices alone."""
    keep: list = []
    cb = sl.c_struct(keep)
    dig = np.zeros((max(z - a, 1), 32), np.uint8)
    bases = np.ascontiguousarray(bases, np.uint64)
    lib().emus_body_hash(ctypes.addressof(cb), a, z, bases.ctypes.data, dig.ctypes.data)
    return dig[: z - a]
