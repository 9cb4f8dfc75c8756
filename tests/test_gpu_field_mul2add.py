"""The gfx950 fe_mul2add program (babble_amd/csrc/field_asm.h, through
tests/mul2add/libmul2addcheck.so) on the device against Python integers: one
launch over 4,096 lanes covering the operand classes of
tests/mul2add_vectors.py (random, weak inputs, the 17th-limb carry and each
rare block), so the hardware's carry and hazard behaviour is exercised, not
only the generator's interpreter (tests/test_field_mul2add.py)."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import mul2add_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "mul2add", "libmul2addcheck.so")
P = V.P

pytestmark = pytest.mark.gpu


def _pack(xs):
    out = np.zeros((len(xs), 8), dtype=np.uint32)
    for i, x in enumerate(xs):
        for k in range(8):
            out[i, k] = (x >> (32 * k)) & V.M32
    return out


def test_mul2add_matches_python_ints():
    if not os.path.exists(LIB):
        pytest.fail("tests/mul2add/libmul2addcheck.so missing: run __graft_entry__.build()")
    import torch  # noqa: F401  (bind the same HIP runtime torch uses, as babble_amd.native does)

    L = ctypes.CDLL(LIB)
    L.m2a_run.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 5
    L.m2a_run.restype = ctypes.c_int
    cls = V.classes(600, seed=3)
    qs = [q for c in cls.values() for q in c]
    assert len(qs) <= 4096 and all(len(c) > 50 for c in cls.values())
    rng = random.Random(4)
    qs += [tuple(rng.getrandbits(256) for _ in range(4)) for _ in range(4096 - len(qs))]  # 16 full blocks
    ops = [_pack([q[k] for q in qs]) for k in range(4)]
    R = np.zeros_like(ops[0])
    assert L.m2a_run(len(qs), *[o.ctypes.data for o in ops], R.ctypes.data) == 0
    out = [sum(int(R[i, k]) << (32 * k) for k in range(8)) for i in range(len(qs))]
    bad = [(i, hex(a), hex(b), hex(x), hex(y), hex(z)) for i, ((a, b, x, y), z) in enumerate(zip(qs, out))
           if (z - (a * b + x * y)) % P]
    assert not bad, bad[:3]
