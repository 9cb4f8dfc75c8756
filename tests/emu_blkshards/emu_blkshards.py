"""ctypes wrapper of tests/emu_blkshards/_build/libbvemublkshards.so: the
rebased BlockBody serialiser (blkjson.h blk_len / blk_emit with BlkBases, what
k_blk_body_hash_rb runs per lane) on the host.  Test infrastructure only."""
from __future__ import annotations

import ctypes
import dataclasses
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_build", "libbvemublkshards.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
        L = ctypes.CDLL(LIB)
        L.emubs_body_hash.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
        L.emubs_body_hash.restype = ctypes.c_int
        _lib = L
    return _lib


def slice_blocks(pb, b0: int, b1: int, i0: int, i1: int):
    """What the shard of blocks [b0, b1) and items [i0, i1) of `pb` ships
    (bv_group_verify_blocks): COPIES of its slices, the values in them
    unchanged, and the bases (blk, hash, tx, txb, itx, rcpt).  The keys stay
    whole."""
    h0, h1 = int(pb.hash_off[3 * b0]), int(pb.hash_off[3 * b1])
    t0, t1 = int(pb.tx_start[b0]), int(pb.tx_start[b1])
    has_tx = len(pb.tx_off) > 1
    x0, x1 = (int(pb.tx_off[t0]), int(pb.tx_off[t1])) if has_tx else (0, 0)

    def frag(off, data):
        if off is None:
            return None, data[:0].copy(), 0
        lo, hi = int(off[b0]), int(off[b1])
        return off[b0:b1 + 1].copy(), data[lo:hi].copy(), lo

    def cut(a, lo, hi):
        return None if a is None else a[lo:hi].copy()

    itx_off, itx_json, itx_base = frag(pb.itx_off, pb.itx_json)
    rcpt_off, rcpt_json, rcpt_base = frag(pb.rcpt_off, pb.rcpt_json)
    s0, s1 = (int(pb.sig_off[i0]), int(pb.sig_off[i1])) if pb.sig_off is not None else (0, 0)
    sl = dataclasses.replace(
        pb, index=pb.index[b0:b1].copy(), round_received=pb.round_received[b0:b1].copy(),
        timestamp=pb.timestamp[b0:b1].copy(), hash_off=pb.hash_off[3 * b0:3 * b1 + 1].copy(),
        hash_bytes=pb.hash_bytes[h0:h1].copy(), hash_nil=cut(pb.hash_nil, 3 * b0, 3 * b1),
        tx_start=pb.tx_start[b0:b1 + 1].copy(),
        tx_off=pb.tx_off[t0:t1 + 1].copy() if has_tx else pb.tx_off[:0].copy(), tx_bytes=pb.tx_bytes[x0:x1].copy(),
        tx_list_nil=cut(pb.tx_list_nil, b0, b1), tx_nil=cut(pb.tx_nil, t0, t1),
        itx_off=itx_off, itx_json=itx_json, rcpt_off=rcpt_off, rcpt_json=rcpt_json,
        item_block=pb.item_block[i0:i1].copy(), item_key=pb.item_key[i0:i1].copy(),
        sig_off=cut(pb.sig_off, i0, i1 + 1), sig_text=cut(pb.sig_text, s0, s1),
        r_be=cut(pb.r_be, i0, i1), s_be=cut(pb.s_be, i0, i1), pre=cut(pb.pre, i0, i1))
    return sl, np.array([b0, h0, t0, x0, itx_base, rcpt_base], np.uint64)


def body_hash(sl, bases: np.ndarray, b0: int, b1: int):
    """(digests [b1 - b0, 32], body lengths [b1 - b0]) of blocks [b0, b1) from
    the shard's slices alone."""
    keep: list = []
    cb = sl.c_struct(keep)
    n = b1 - b0
    dig = np.zeros((max(n, 1), 32), np.uint8)
    lens = np.zeros(max(n, 1), np.uint64)
    bases = np.ascontiguousarray(bases, np.uint64)
    rc = lib().emubs_body_hash(ctypes.addressof(cb), b0, b1, bases.ctypes.data, dig.ctypes.data, lens.ctypes.data)
    assert rc == 0, "the SHA sink took another byte count than blk_len"
    return dig[:n], lens[:n]
