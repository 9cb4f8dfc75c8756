"""k_sinv's block-level batch inversion (BV_SINV_BLOCK) on the device.

tests/sinvblock/libsinvblockcheck.so launches both forms of k_sinv
(babble_amd/csrc/sinv_kernels.h: one inversion per lane, and k_sinv_block)
with the launcher's geometry on the cases of tests/test_sinv_block.py
(n x M, with unusable items first, last and alone in a lane, a whole lane and
a whole block of them); w must be equal word for word on every usable item,
and s w = R (mod N) in Python integers.

Then two batches through the public device entry, both with a ragged last
block: 65,537 + 64 + 5 items (M = 2; a latency shape, for which the launcher
keeps the per-lane kernel) and 3 x 65,536 + 64 + 5 items (M = 4, past the
latency shapes: k_sinv_block).
"""
import ctypes
import os

import numpy as np
import pytest

from babble_amd import synth
from tests import test_sinv_block as cpu
from tests.test_gpu import check_against_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "sinvblock", "libsinvblockcheck.so")

pytestmark = pytest.mark.gpu

_LIB = []


def lib():
    if not _LIB:
        if not os.path.exists(LIB):
            pytest.fail("tests/sinvblock/libsinvblockcheck.so missing: run __graft_entry__.build()")
        import torch  # noqa: F401  (bind the same HIP runtime torch uses, as babble_amd.native does)

        L = ctypes.CDLL(LIB)
        L.sinvblock_run.argtypes = [ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 4
        L.sinvblock_run.restype = ctypes.c_int
        _LIB.append(L)
    return _LIB[0]


@pytest.mark.parametrize("m", cpu.MS)
def test_both_kernels_give_the_same_w(m):
    L = lib()
    for n in cpu.SIZES:
        items, bad = cpu.CASES[(n, m)]
        s_be = np.frombuffer(b"".join(s.to_bytes(32, "big") for s, _ in items), np.uint8).copy()
        pre = np.array([p for _, p in items], np.uint8)
        w_lane = np.zeros((n, 8), np.uint32)
        w_block = np.zeros((n, 8), np.uint32)
        assert L.sinvblock_run(n, m, s_be.ctypes.data, pre.ctypes.data, w_lane.ctypes.data, w_block.ctypes.data) == 0
        usable = np.array([i for i in range(n) if i not in bad], np.int64)
        assert usable.size == n - len(bad)
        differ = np.flatnonzero((w_lane[usable] != w_block[usable]).any(axis=1))
        assert differ.size == 0, (n, m, usable[differ][:8])
        for i in usable:
            w = sum(int(w_block[i, k]) << (32 * k) for k in range(8))
            assert w < cpu.N and w * items[i][0] % cpu.N == cpu.R % cpu.N, (n, m, int(i))


@pytest.mark.parametrize("n, m", [(65537 + 64 + 5, 2), (3 * 65536 + 64 + 5, 4)])
def test_device_entry_ragged_block(n, m):
    from babble_amd.verifier import Verifier

    assert min(16, -(-n // 65536)) == m  # bv_api.cpp's rule for M
    assert -(-n // m) % 256 != 0  # the last block is ragged
    assert (n > 131072) == (m == 4)  # BV_LAT_MAX_ITEMS: only the larger batch takes k_sinv_block
    b = synth.adversarial(n, seed=10, n_creators=8)
    v = Verifier(device=0)
    try:
        res = check_against_oracle(v, b, device_api=True)
        counts = np.bincount(res.status, minlength=4)
        assert counts[0] > 0 and counts[1] > 0, counts
    finally:
        v.close()
