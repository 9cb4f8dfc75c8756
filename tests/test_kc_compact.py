"""The compact key-cache geometry KC18 (BV_F_KEY_CACHE | BV_F_KC_COMPACT: 18-bit
signed windows x 8 over each GLV half from 9-bit sub-tables, 67.1 MB per key)
without a device: the flag rules of bv_create, the edge vectors of
tests/edge_vectors_kc18.py, and the table build and the key part of the verify
replayed on the CPU from the device's own source.

tests/kccompact/kccompact_main.cpp is a stand-alone host program (its own
main, plain clang, nothing loaded into Python).  Per key it replays
k_table_bases, k_table_fill<9, 16, false> and k_table_pair_kc<18, 9, 8> lane
by lane into a patterned buffer between guard words, prints the named table
slots, and runs each vector's key part through verify_item_qfirst<18, 8, LAT>
for both LAT values against an allocation of exactly the table's size.

Vectors the program takes: ALL of edge_vectors_kc18.vectors() — every sign
pair of every rotation, the top-window, zero / equal-half and from-identity
shapes, b/max, and families d and e — 86 keys at ~0.6 s a key.  The program is
also built with -fsanitize=address,undefined and run on two keys (a rotation's
and b/max's largest half).
"""
import ctypes
import os
import random
import subprocess

import pytest

from babble_amd import native
from oracle import gosemantics as gs
from tests import edge_vectors as ev
from tests import edge_vectors_kc18 as kv

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kccompact")
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
P, N = gs.P, gs.N
W, NWIN, L = 18, 8, 9
ENT = 1 << (W - 1)
SLOT_COUNT = NWIN * ENT + 1
TABLE_BYTES = SLOT_COUNT * 64
FILL = "a5a5a5a5" * 8

SLOTS = ([1, 2, (1 << L) - 1, 1 << L, (1 << L) + 1, ENT - 1] + [ENT * j for j in range(1, NWIN + 1)] +
         [ENT * (NWIN - 1) + d for d in (1, 2, 3, 4, 5)])


def slot_scalar(slot):
    """The multiple of Q that table slot j ENT + d holds (d = 0: the digit
    2^(W-1) of window j - 1; j = NWIN: the pad entry after the top window)."""
    j, d = divmod(slot, ENT)
    return d << (W * j) if d else ENT << (W * (j - 1))


# ---------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------
def test_flag_rules():
    import torch

    L_ = native.lib()
    assert native.F_KC_COMPACT == 4
    ctx = ctypes.c_void_p()
    # the compact geometry is one of the key cache's: alone it is an argument error
    assert L_.bv_create(ctypes.byref(ctx), 0, native.F_KC_COMPACT) == native.BV_E_ARGS and not ctx.value
    assert L_.bv_create(ctypes.byref(ctx), 0, native.F_KC_COMPACT | native.F_K8) == native.BV_E_ARGS and not ctx.value
    assert L_.bv_create(ctypes.byref(ctx), 0, 0x80) == native.BV_E_ARGS and not ctx.value
    assert L_.bv_create(ctypes.byref(ctx), 0, 0x80 | native.F_KEY_CACHE | native.F_KC_COMPACT) == native.BV_E_ARGS
    assert L_.bv_abi_version() == 6  # additive: a bit that was an error before
    if not torch.cuda.is_available():
        # with the cache the flag passes the flag checks and reaches the device probe
        rc = L_.bv_create(ctypes.byref(ctx), 0, native.F_KEY_CACHE | native.F_KC_COMPACT)
        assert rc == native.BV_E_NODEVICE and not ctx.value


def test_header_documents_the_tier():
    text = open(os.path.join(ROOT, "include", "babbleverify.h")).read()
    assert "#define BV_F_KC_COMPACT 4u" in text
    assert "#define BV_F_KNOWN (BV_F_KEY_CACHE | BV_F_K8 | BV_F_KC_COMPACT)" in text
    assert f"{TABLE_BYTES:,}" in text and TABLE_BYTES == 67_108_928
    assert 96e9 // TABLE_BYTES == 1430 and "1430" in text
    assert 0.25e9 // TABLE_BYTES == 3


# ---------------------------------------------------------------------------
# vectors
# ---------------------------------------------------------------------------
def test_vectors_halves_are_the_splits():
    own = kv.own().out
    assert len(own) == 60 and len({v.pub for v in own}) == 60
    for v in own:
        assert ev.glv_halves(v.u2) == v.meta["k"], v.tag
        assert v.expect == ev.ACCEPT
    # the patterns the split never returns: the top window's digit 2 next to an empty half
    assert sorted(t for t, _, _ in kv.dropped()) == ["b/KC18/top-below-sub/k1", "b/KC18/top-below-sub/k2"]
    vs = kv.vectors()
    for v, st in zip(vs, kv.direct_statuses()):
        assert st == v.expect, v.tag
    fams = {v.family for v in vs}
    assert fams == {"b", "d", "e"}
    assert sum(v.tag.startswith("b/max/") for v in vs) >= 10
    assert {v.tag for v in ev.vectors() if v.family in "de"} <= {v.tag for v in vs}


def test_vectors_reach_every_window_class():
    seen = kv.halves_classes()
    cycle = set(ev._SIGNED_CYCLE)
    assert seen[0] >= cycle - {"full+carry"}  # window 0 has no carry in
    for j in range(1, NWIN - 1):
        assert seen[j] >= cycle, (j, cycle - seen[j])
    # the top window: 2 live bits; digits 0, 1 (the rotations, top-one) and 2, 3 (b/max)
    assert seen[NWIN - 1] >= {"zero", "one", "below-sub"}
    tops = set()
    for v in kv.vectors():
        for k in ev.glv_halves(v.u2):
            d = ev.signed_digits(abs(k), W, NWIN)
            tops.add(d[NWIN - 1])
            assert all(-ENT < x <= ENT for x in d) and 0 <= d[NWIN - 1] <= 4
    assert tops == {0, 1, 2, 3}


# ---------------------------------------------------------------------------
# the CPU replay
# ---------------------------------------------------------------------------
def _compile(name, extra):
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    exe = os.path.join(HERE, "_build", name)
    subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + extra +
                   [os.path.join(HERE, "kccompact_main.cpp"), "-o", exe], check=True, cwd=ROOT)
    return exe


def _inputs(tmp, idx, skipped=True):
    """Key and vector files for the vectors at `idx`: one key per distinct
    pubkey, in order of first use, and (`skipped`) one key with status 2."""
    vs = kv.vectors()
    keys, lines = [], []
    for i in idx:
        v = vs[i]
        q = gs.Unmarshal(v.pub)
        if q not in keys:
            keys.append(q)
        lines.append((keys.index(q), i))
    status = [0] * len(keys)
    if skipped:
        keys.append(gs.scalar_mult(random.Random(0x18).randrange(1, N), gs.G))
        status.append(2)
    kp, vp = str(tmp / "keys.txt"), str(tmp / "vectors.txt")
    with open(kp, "w") as f:
        for (x, y), st in zip(keys, status):
            f.write(f"{x:064x} {y:064x} {st}\n")
    with open(vp, "w") as f:
        for b, i in lines:
            f.write(f"{b} {vs[i].r:064x} {vs[i].s:064x}\n")
    return kp, vp, keys, status, [i for _, i in lines]


def _check(stdout, keys, status, order):
    """Every line of the program's output against Python integers."""
    vs = kv.vectors()
    lines = [ln.split() for ln in stdout.splitlines()]
    entries = rqs = 0
    for ln in lines:
        b = int(ln[1])
        live = status[b] == 0
        if ln[0] == "STORES":
            stores, max_slot, off = int(ln[2]), int(ln[3]), int(ln[4])
            # windows 0..6 whole, the top window's one live block of 4096, the pad the highest
            assert (stores, max_slot, off) == ((7 * ENT + 4096, ENT * NWIN, 0) if live else (0, 0, 0)), ln
        elif ln[0] == "GUARD":
            changed, pattern, words = int(ln[2]), int(ln[3]), int(ln[4])
            assert changed == 0 and words == SLOT_COUNT * 16, ln
            # a skipped key's buffer is untouched; a built one keeps the pattern in the never-stored slots only
            assert pattern == (16 * (SLOT_COUNT - 7 * ENT - 4096) if live else words), ln
        elif ln[0] == "E":
            slot, x, y = int(ln[2]), ln[3], ln[4]
            if not live:
                assert (x, y) == (FILL, FILL), "a skipped key's table was written"
            else:
                assert (int(x, 16), int(y, 16)) == gs.scalar_mult(slot_scalar(slot), keys[b]), (b, slot)
            entries += 1
        elif ln[0] == "LOOKUP":
            assert int(ln[3]) < int(ln[4]) == SLOT_COUNT, ln
            assert int(ln[3]) <= ENT * (NWIN - 1) + 4, ln  # the top window's digit is at most 2^2
        elif ln[0] == "RQ":
            v = vs[order[int(ln[2])]]
            want = gs.scalar_mult(v.u2, keys[b])
            assert want is not None and ln[4] == "0", v.tag  # u2 Q is never the identity (0 < u2 < N)
            assert (int(ln[5], 16), int(ln[6], 16)) == want, (v.tag, "LAT" if ln[3] == "1" else "pipelined")
            rqs += 1
        else:
            raise AssertionError(ln)
    assert entries == len(keys) * len(SLOTS) and rqs == 2 * len(order)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    exe = _compile("kccompact", [])
    kp, vp, keys, status, order = _inputs(tmp_path_factory.mktemp("kccompact"), range(len(kv.vectors())))
    r = subprocess.run([exe, kp, vp] + [str(s) for s in SLOTS], capture_output=True, text=True, timeout=900)
    return r, keys, status, order


def test_named_slots_are_in_the_table():
    assert max(SLOTS) == ENT * NWIN == SLOT_COUNT - 1
    assert [slot_scalar(ENT * j) for j in (1, NWIN)] == [ENT, ENT << (W * (NWIN - 1))]
    assert slot_scalar(ENT * (NWIN - 1) + 5) == 5 << 126


def test_build_and_key_part_on_the_cpu(replay):
    r, keys, status, order = replay
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(keys) == 87 and status.count(2) == 1
    _check(r.stdout, keys, status, order)


def test_build_and_key_part_under_sanitizers(tmp_path):
    exe = _compile("kccompact_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    vs = kv.vectors()
    tags = {"b/KC18/rot7/-+", "b/max/k1=0x80000000000000000000000000000000,k2=0"}
    idx = [i for i, v in enumerate(vs) if v.tag in tags]
    assert len(idx) == 2
    kp, vp, keys, status, order = _inputs(tmp_path, idx, skipped=False)
    r = subprocess.run([exe, kp, vp] + [str(s) for s in SLOTS], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    _check(r.stdout, keys, status, order)
