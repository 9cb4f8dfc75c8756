"""ctypes wrapper of tests/emu_itx/_build/libbvemuitx.so: the device's
streaming InternalTransaction paths (itxjson.h into the EvjSha sink, what
k_itx_body_hash and k_ev_body_hash_itx run per lane) and the length functions
on the host.  Test infrastructure only."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_build", "libbvemuitx.so")
FUZZ = os.path.join(_HERE, "_build", "itxfuzz")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
        L = ctypes.CDLL(LIB)
        P, U = ctypes.c_void_p, ctypes.c_uint64
        for f in (L.emui_itx_body_hash, L.emui_ev_body_hash):
            f.argtypes = [P, U, U, P]
            f.restype = None
        L.emui_lens.argtypes = [P, ctypes.c_int, U, U, P, P]
        L.emui_lens.restype = None
        L.emui_ppos.argtypes = [P, U, P]
        L.emui_ppos.restype = None
        L.emui_string.argtypes = [ctypes.c_char_p, U, P, U, P]
        L.emui_string.restype = U
        _lib = L
    return _lib


def _hash(fn, xb, n) -> np.ndarray:
    keep: list = []
    cb = xb.c_struct(keep)
    dig = np.zeros((max(n, 1), 32), np.uint8)
    fn(ctypes.addressof(cb), 0, n, dig.ctypes.data)
    return dig[:n]


def itx_body_hash(xb) -> np.ndarray:
    """Digests [n_itx, 32] of every ITX body of an events.PackedEventItxBatch."""
    return _hash(lib().emui_itx_body_hash, xb, xb.n_itx)


def ev_body_hash(xb) -> np.ndarray:
    """Digests [n, 32] of every event body (in-batch parents as 64 '0')."""
    return _hash(lib().emui_ev_body_hash, xb, xb.n_events)


def lens(xb, kind: int):
    """(the *_len function, the emitted byte count) per ITX (kind 0: body, 1:
    list element) or per event (kind 2)."""
    keep: list = []
    cb = xb.c_struct(keep)
    n = xb.n_events if kind == 2 else xb.n_itx
    a, b = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    lib().emui_lens(ctypes.addressof(cb), kind, 0, n, a.ctypes.data, b.ctypes.data)
    return a[:n], b[:n]


def ppos(xb, e: int):
    keep: list = []
    cb = xb.c_struct(keep)
    pp = np.zeros(2, np.uint32)
    lib().emui_ppos(ctypes.addressof(cb), e, pp.ctypes.data)
    return int(pp[0]), int(pp[1])


def string(s: bytes):
    """(gojson_string's output, gojson_string_len)."""
    out = np.zeros(6 * len(s) + 2, np.uint8)
    w = ctypes.c_uint64()
    n = lib().emui_string(bytes(s), len(s), out.ctypes.data, out.size, ctypes.byref(w))
    return out[: w.value].tobytes(), int(n)


def fuzz_exe() -> str:
    """The ASan + UBSan fuzz driver (built on first use); run it as a subprocess."""
    subprocess.run(["make", "-s", "-C", _HERE, "fuzz"], check=True)
    return FUZZ
