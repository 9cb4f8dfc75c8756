"""ctypes wrapper of tests/emu_blocks/_build/libbvemublocks.so: the device's
streaming BlockBody path (blkjson.h blk_emit into the EvjSha sink, what
k_blk_body_hash runs per lane) on the host.  Test infrastructure only."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_build", "libbvemublocks.so")
FUZZ = os.path.join(_HERE, "_build", "blkfuzz")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
        L = ctypes.CDLL(LIB)
        L.emub_body_hash.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        L.emub_body_hash.restype = None
        L.emub_body_len.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        L.emub_body_len.restype = None
        _lib = L
    return _lib


def body_hash(pb) -> np.ndarray:
    """Digests [n, 32] of every block of a batch.PackedBlockBatch."""
    keep: list = []
    cb = pb.c_struct(keep)
    n = pb.n_blocks
    dig = np.zeros((max(n, 1), 32), np.uint8)
    lib().emub_body_hash(ctypes.addressof(cb), 0, n, dig.ctypes.data)
    return dig[:n]


def body_len(pb) -> np.ndarray:
    keep: list = []
    cb = pb.c_struct(keep)
    n = pb.n_blocks
    lens = np.zeros(max(n, 1), np.uint64)
    lib().emub_body_len(ctypes.addressof(cb), 0, n, lens.ctypes.data)
    return lens[:n]


def fuzz_exe() -> str:
    """The ASan + UBSan fuzz driver (built on first use); run it as a subprocess."""
    subprocess.run(["make", "-s", "-C", _HERE, "fuzz"], check=True)
    return FUZZ
