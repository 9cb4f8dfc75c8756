"""The K12 sub-table fill from shared multiples (verify_core.h
BV_FILL_SHARED: k_fill_multiples + k_table_fill_shared) against the per-entry
double-and-add of k_table_fill, byte for byte, and against Python integers.

tests/fillshared/fillshared_main.cpp is a stand-alone host program compiled
from the device's own source (nothing is loaded into Python): it replays the
kernels lane by lane and builds each key's sub-tables and K12 table both
ways.  Keys: the generator itself, a seeded random key, a key whose x has a
high top limb, and one the kernels skip (status != KS_OK), whose memory must
stay untouched.
"""
import os
import random
import subprocess

import pytest

from oracle import gosemantics as gs

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fillshared")
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
P, N = gs.P, gs.N
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
W, NWIN, L, NSUB = 12, 11, 6, 22
ENT = 1 << (W - 1)
FILL = "a5a5a5a5" * 8


def keys():
    rng = random.Random(0xF111)
    q1 = gs.scalar_mult(rng.randrange(1, N), gs.G)
    while True:  # x >= 2^256 - 2^224: a top limb of all ones
        q2 = gs.scalar_mult(rng.randrange(1, N), gs.G)
        if q2[0] >> 248 == 0xFF:
            break
    skipped = gs.scalar_mult(rng.randrange(1, N), gs.G)
    return [(gs.G, 0), (q1, 0), (skipped, 2), (q2, 0)]


def slot_scalar(slot):
    """The multiple of Q that K12 table slot j ENT + d holds (d = 0: the
    digit 2^(W-1) of window j - 1)."""
    j, d = divmod(slot, ENT)
    return d << (W * j) if d else ENT << (W * (j - 1))


SLOTS = [1, 2, 63, 64, 65, 2047, 2048, 2049, ENT * 5 + 1984, ENT * 5 + 2047, ENT * 6, ENT * 10 + 1, ENT * 10 + 256,
         ENT * 10 + 257, ENT * 11]


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    exe = os.path.join(HERE, "_build", "fillshared")
    subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(HERE, "fillshared_main.cpp"), "-o", exe], check=True, cwd=ROOT)
    path = str(tmp_path_factory.mktemp("fillshared") / "keys.txt")
    with open(path, "w") as f:
        for (x, y), st in keys():
            f.write(f"{x:064x} {y:064x} {st}\n")
    r = subprocess.run([exe, path] + [str(s) for s in SLOTS], capture_output=True, text=True, timeout=600)
    return r.returncode, [ln.split() for ln in r.stdout.splitlines()], r.stderr


def test_tables_are_byte_identical(result):
    rc, lines, err = result
    by = {ln[0]: ln[1:] for ln in lines if ln[0] != "E"}
    live = 3 * (11 * 64 + 11 * 33)
    assert by["SUB"] == [str(live), "0"], (by, err)
    assert by["TABLE"][1] == "0" and int(by["TABLE"][0]) == 4 * 2 * ((NWIN * ENT + 1) * 16), (by, err)
    # the new fill writes the live entries only: the odd sub-tables above
    # x = 32 and the skipped key keep the buffer's pattern
    dead = (3 * 11 * 31 + NSUB * 64) * 16
    assert by["DEAD"] == [str(dead), str(dead)], (by, err)
    assert rc == 0, err


def test_entries_are_the_multiples_of_the_key(result):
    rc, lines, err = result
    ks = keys()
    seen = 0
    for ln in lines:
        if ln[0] != "E":
            continue
        b, slot, x, y, px = int(ln[1]), int(ln[2]), ln[3], ln[4], ln[5]
        (q, st) = ks[b]
        if st != 0:
            assert (x, y, px) == (FILL, FILL, FILL), "a skipped key's table was written"
            continue
        want = gs.scalar_mult(slot_scalar(slot), q)
        assert (int(x, 16), int(y, 16)) == want, (b, slot)
        assert int(px, 16) == BETA * want[0] % P, (b, slot)
        seen += 1
    assert seen == 3 * len(SLOTS)
