"""ctypes wrapper of tests/emu_fields/_build/libbvemufields.so: the device's
streaming whole-event path (bsigjson.h into the EvjSha sink, what
k_ev_body_hash_fields runs per lane) and the length functions on the host.
Test infrastructure only."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_build", "libbvemufields.so")
FUZZ = os.path.join(_HERE, "_build", "fieldsfuzz")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
        L = ctypes.CDLL(LIB)
        P, U = ctypes.c_void_p, ctypes.c_uint64
        L.emuf_ev_body_hash.argtypes = [P, U, U, P]
        L.emuf_ev_body_hash.restype = None
        L.emuf_lens.argtypes = [P, ctypes.c_int, U, U, P, P, P]
        L.emuf_lens.restype = None
        L.emuf_ppos.argtypes = [P, U, P]
        L.emuf_ppos.restype = None
        _lib = L
    return _lib


def ev_body_hash(fb) -> np.ndarray:
    """Digests [n, 32] of every event body of an events.PackedEventFieldsBatch
    (in-batch parents as 64 '0')."""
    keep: list = []
    cb = fb.c_struct(keep)
    n = fb.n_events
    dig = np.zeros((max(n, 1), 32), np.uint8)
    lib().emuf_ev_body_hash(ctypes.addressof(cb), 0, n, dig.ctypes.data)
    return dig[:n]


def lens(fb, kind: int):
    """(the *_len function, the emitted byte count) per block signature (kind
    0: its list element) or per event (kind 1)."""
    keep: list = []
    cb = fb.c_struct(keep)
    n = fb.n_events if kind == 1 else fb.n_bsig
    owner = np.repeat(np.arange(fb.n_events, dtype=np.uint64), np.diff(fb.bsig_start).astype(np.int64))
    owner = np.ascontiguousarray(np.append(owner, np.uint64(0)))
    a, b = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    lib().emuf_lens(ctypes.addressof(cb), kind, 0, n, owner.ctypes.data, a.ctypes.data, b.ctypes.data)
    return a[:n], b[:n]


def ppos(fb, e: int):
    keep: list = []
    cb = fb.c_struct(keep)
    pp = np.zeros(2, np.uint32)
    lib().emuf_ppos(ctypes.addressof(cb), e, pp.ctypes.data)
    return int(pp[0]), int(pp[1])


def fuzz_exe() -> str:
    """The ASan + UBSan fuzz driver (built on first use); run it as a subprocess."""
    subprocess.run(["make", "-s", "-C", _HERE, "fuzz"], check=True)
    return FUZZ
