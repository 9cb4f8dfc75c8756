"""KC18 table leaves in the small-batch kernel (bv_kc_small_tables), without a
device: the new entry point's ABI, and the table lanes of k_small's warm tree
replayed on the CPU from the device's own source.

tests/kcsmall/kcsmall_main.cpp is a stand-alone host program (its own main,
plain clang, nothing loaded into Python).  It runs small_table_leaf<KW, KNWIN>
of verify_core.h — the function k_small's lanes 10.. call: lane -> (GLV half,
window), signed recoding, table address, phi and sign — for every table lane
of one item, against a table of exactly the geometry's size holding the
pattern everywhere but in the slots this file names.

Per vector this file computes, in Python integers, the halves of u2
(edge_vectors.glv_halves), their signed digits (edge_vectors.signed_digits)
and for each non-zero digit d of window j the slot j ENT + |d| with the affine
point |d| 2^(W j) Q.  The program must read exactly those slots for the
non-zero leaves (and nothing outside the table, nothing past the top window's
digit 4), and the sum of its leaves must be u2 Q.

Vectors: ALL of edge_vectors_kc18.vectors() for <18, 8> (every one reaches the
math: valid key, 0 < r, s < N); five of them again for <22, 6>, the geometry
the kernel had before it became a template (an 805 MB table buffer, one run).
The program is also built with -fsanitize=address,undefined and run on two
vectors.
"""
import ctypes
import os
import subprocess

import pytest

from babble_amd import native
from oracle import gosemantics as gs
from tests import edge_vectors as ev
from tests import edge_vectors_kc18 as kv

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kcsmall")
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
N = gs.N
GEOM = {18: 8, 22: 6}  # W -> windows per GLV half
GNWIN = 10  # the G leaves come first: table lane q is lane 10 + q
SAN_TAGS = ("b/KC18/rot7/-+", "b/max/k1=0x80000000000000000000000000000000,k2=0")
KC22_TAGS = SAN_TAGS + ("b/KC18/rot0/++", "b/KC18/rot3/+-", "b/KC18/rot5/--")


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "babbleverify.h")).read()
    assert "int bv_kc_small_tables(bv_ctx *ctx, int on);" in text
    assert "#define BV_ABI_VERSION 6" in text


def test_library_exports_it():
    assert "bv_kc_small_tables" in native.EXPORTS
    L_ = native.lib()
    fn = getattr(L_, "bv_kc_small_tables")  # AttributeError: not exported
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 2
    assert L_.bv_abi_version() == 6  # additive


def test_null_context_is_an_argument_error():
    assert native.lib().bv_kc_small_tables(None, 1) == native.BV_E_ARGS
    assert native.lib().bv_kc_small_tables(None, 0) == native.BV_E_ARGS


# ---------------------------------------------------------------------------
# the CPU replay
# ---------------------------------------------------------------------------
def reaches_math(v):
    return gs.Unmarshal(v.pub) is not None and 0 < v.r < N and 0 < v.s < N


def slots_of(v, W):
    """{slot: affine point} a table of geometry W must hold for v's item: one
    per non-zero signed digit of either half of u2 (the halves share the one
    stored table; phi and the signs are the leaf's work)."""
    NWIN, ENT = GEOM[W], 1 << (W - 1)
    q = gs.Unmarshal(v.pub)
    out = {}
    for k in ev.glv_halves(v.u2):
        for j, d in enumerate(ev.signed_digits(abs(k), W, NWIN)):
            if d:
                out[j * ENT + abs(d)] = gs.scalar_mult(abs(d) << (W * j), q)
    return out


def _compile(name, extra):
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    exe = os.path.join(HERE, "_build", name)
    subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + extra +
                   [os.path.join(HERE, "kcsmall_main.cpp"), "-o", exe], check=True, cwd=ROOT)
    return exe


def _run(exe, tmp, cases):
    """cases: (W, vector) in program order -> (CompletedProcess, [slots per case])."""
    path, stored = str(tmp / "vectors.txt"), []
    with open(path, "w") as f:
        for W, v in cases:
            s = slots_of(v, W)
            stored.append(s)
            f.write(f"{W} {v.u2:064x} {len(s)} " + " ".join(f"{k} {x:064x} {y:064x}" for k, (x, y) in s.items()) + "\n")
    return subprocess.run([exe, path], capture_output=True, text=True, timeout=600), stored


def _check(r, cases, stored):
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    leaves = [[] for _ in cases]
    sums, guards = {}, {}
    for ln in (x.split() for x in r.stdout.splitlines()):
        if ln[0] == "LEAF":
            leaves[int(ln[1])].append((int(ln[2]), int(ln[3]), ln[4] == "1", ln[5] == "1"))
        elif ln[0] == "SUM":
            sums[int(ln[1])] = (ln[2], int(ln[3], 16), int(ln[4], 16))
        elif ln[0] == "GUARD":
            guards[int(ln[1])] = (int(ln[2]), int(ln[3]))
        else:
            raise AssertionError(ln)
    assert guards == {W: (0, 0) for W in {W for W, _ in cases}}
    for i, (W, v) in enumerate(cases):
        NWIN, ENT = GEOM[W], 1 << (W - 1)
        assert [lane for lane, _, _, _ in leaves[i]] == list(range(GNWIN, GNWIN + 2 * NWIN)), v.tag
        digits = [d for k in ev.glv_halves(v.u2) for d in ev.signed_digits(abs(k), W, NWIN)]
        read = set()
        for (lane, slot, zero, is_stored), d in zip(leaves[i], digits):
            j = (lane - GNWIN) % NWIN
            assert zero == (d == 0) and slot == j * ENT + abs(d) and slot < NWIN * ENT + 1, (v.tag, lane)
            if not zero:
                assert is_stored and slot in stored[i], (v.tag, lane)
                read.add(slot)
            if W == 18 and j == NWIN - 1:
                assert slot <= 7 * ENT + 4, (v.tag, lane)  # the top window's one stored block, digits 0..4
        assert read == set(stored[i]), v.tag  # every stored slot was some leaf's
        want = gs.scalar_mult(v.u2, gs.Unmarshal(v.pub))
        assert want is not None and sums[i][0] == "0", v.tag  # u2 Q is never the identity (0 < u2 < N)
        assert sums[i][1:] == want, (v.tag, W)


def test_every_vector_reaches_the_math():
    vs = kv.vectors()
    assert len(vs) >= 80 and all(reaches_math(v) for v in vs)
    tags = {v.tag for v in vs}
    assert set(KC22_TAGS) <= tags


def test_warm_leaves_on_the_cpu(tmp_path):
    """<18, 8> on every vector, then <22, 6> on five."""
    vs = [v for v in kv.vectors() if reaches_math(v)]
    cases = [(18, v) for v in vs] + [(22, v) for v in vs if v.tag in KC22_TAGS]
    assert sum(W == 22 for W, _ in cases) == len(KC22_TAGS)
    r, stored = _run(_compile("kcsmall", []), tmp_path, cases)
    _check(r, cases, stored)
    tops = {max(s) - 7 * (1 << 17) for (W, _), s in zip(cases, stored) if W == 18 and max(s) > 7 * (1 << 17)}
    assert tops == {1, 2, 3}  # the top window's non-zero digits the vectors offer


def test_warm_leaves_under_sanitizers(tmp_path):
    exe = _compile("kcsmall_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    cases = [(18, v) for v in kv.vectors() if v.tag in SAN_TAGS]
    assert len(cases) == 2
    r, stored = _run(exe, tmp_path, cases)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    _check(r, cases, stored)
