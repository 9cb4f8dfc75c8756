"""BV_DEFER_EXC (one exception test per item) and BV_FUSED_Y3 on the CPU.

tests/deferexc/deferexc_main.cpp compiles verify_core.h for the host (through
the host emulator's table builders) as a stand-alone program, with both knobs
at 1 and at 0, and once under AddressSanitizer + UBSan; nothing is loaded into
Python.  Over the golden items, the chosen-scalar edge vectors and the crafted
exception vectors of tests/defer_vectors.py both builds must give, item for
item, the C oracle's status in the device entry's order (verify_item_g, then
verify_item_q) and in the host entries' order (verify_item_qfirst, then
verify_item_gfinish), and stored partial sums R_G / R_Q that are the same
group elements.  The second, checked pass (a counter in the host build) must
be taken by every crafted vector, by no golden accept, and never with the
knob at 0.  The program's "unit" section runs the unchecked additions
(general, trimmed and the affine second step) on accumulators equal to +-the
entry: ZZ3 == 0 there, and != 0 with the checked form's point elsewhere.  (A
real digit sequence cannot reach the affine step with P == 0: window 1's
entry is at least 2^12 times window 0's, so only the unit section covers it.)
"""
import os
import subprocess

import numpy as np
import pytest

from tests import defer_vectors as dv
from tests import edge_vectors as ev
from tests.emu import emu
from tests.helpers import golden_items_batch, load

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deferexc")
ROOT = os.path.dirname(os.path.dirname(HERE))
BUILD = os.path.join(HERE, "_build")
LLVM = os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin")
P, N = ev.P, ev.N
# the emulator's 16-bit generator geometry (a 64 MB table)
GEOM = ["-DBV_GW=16", "-DBV_GNWIN=17", "-DBV_GL=8", "-DBV_GNSUB=34"]
CSRC = os.path.join(ROOT, "babble_amd", "csrc")


def _build(name, knobs, extra):
    os.makedirs(os.path.join(BUILD, name), exist_ok=True)
    flags = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + GEOM + knobs + extra
    objs = []
    for src, lang, std in ((os.path.join(HERE, "deferexc_main.cpp"), "c++", "-std=c++17"),
                           (os.path.join(CSRC, "hostsha.cpp"), "c++", "-std=c++17"),
                           (os.path.join(CSRC, "hostdag.cpp"), "c++", "-std=c++17"),
                           (os.path.join(ROOT, "oracle", "oracle.c"), "c", "-std=c11")):
        obj = os.path.join(BUILD, name, os.path.basename(src) + ".o")
        cc = os.path.join(LLVM, "clang++" if lang == "c++" else "clang")
        subprocess.run([cc, "-x", lang, std] + flags + ["-c", src, "-o", obj], check=True, cwd=ROOT)
        objs.append(obj)
    exe = os.path.join(BUILD, name, "deferexc")
    subprocess.run([os.path.join(LLVM, "clang++")] + extra + ["-o", exe] + objs + ["-lpthread"], check=True)
    return exe


@pytest.fixture(scope="module")
def exes():
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    return {"on": _build("on", ["-DBV_DEFER_EXC=1", "-DBV_FUSED_Y3=1"], ["-O2"]),
            "off": _build("off", ["-DBV_DEFER_EXC=0", "-DBV_FUSED_Y3=0"], ["-O2"]),
            "asan": _build("asan", ["-DBV_DEFER_EXC=1", "-DBV_FUSED_Y3=1"], san)}


@pytest.fixture(scope="module")
def inputs():
    """(batch, kinds): kinds[i] is ('golden', item) / ('edge', Vector) /
    ('crafted', tag) of item i."""
    from babble_amd.batch import BatchBuilder

    bb = BatchBuilder()
    kinds = []
    for it in load("golden_items.json"):
        bb.add_item_raw(bb.add_msg(bytes.fromhex(it["body"])), bb.add_key(bytes.fromhex(it["pub"])), it["pre"],
                        bytes.fromhex(it["r"]), bytes.fromhex(it["s"]))
        kinds.append(("golden", it))
    for v in ev.vectors():
        bb.add_item_raw(bb.add_msg(v.body), bb.add_key(v.pub), 0, v.r.to_bytes(32, "big"), v.s.to_bytes(32, "big"))
        kinds.append(("edge", v))
    for tag, body, pub, r, s in dv.vectors():
        bb.add_item_raw(bb.add_msg(body), bb.add_key(pub), 0, r.to_bytes(32, "big"), s.to_bytes(32, "big"))
        kinds.append(("crafted", tag))
    return bb.pack(), kinds


def _run(exe, arrs, tmp_path, name):
    path = str(tmp_path / f"{name}.bin")
    emu.dump_batch(path, arrs)
    r = subprocess.run([exe, path, "8"], capture_output=True, text=True, timeout=900,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, (name, r.stdout[-1000:] + r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0].startswith("unit ") and int(lines[0].split()[1]) >= 9 * 20
    return [ln.split() for ln in lines[1:]]


def _affine(tok):
    """None (the identity), 'unset' (the item never reached the math) or (x, y)."""
    X, Y, ZZ, ZZZ = (int(t, 16) for t in tok[:4])
    if int(tok[4]):
        return None
    if ZZ == 0:
        return "unset"
    assert pow(ZZ, 3, P) == ZZZ * ZZZ % P
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


def test_knobs_on_and_off_agree_with_the_oracle(exes, inputs, tmp_path):
    batch, kinds = inputs
    on = _run(exes["on"], batch.as_dict(), tmp_path, "on")
    off = _run(exes["off"], batch.as_dict(), tmp_path, "off")
    assert len(on) == len(off) == len(kinds)
    _, expected, _ = golden_items_batch()
    want = list(expected) + list(ev.direct_statuses())
    redo_q, redo_gf = set(), set()
    for i, (a, b) in enumerate(zip(on, off)):
        what = (i, kinds[i][0], kinds[i][1] if kinds[i][0] == "crafted" else getattr(kinds[i][1], "tag", ""))
        oracle = int(a[1])
        assert a[1:4] == [a[1]] * 3 and b[1:4] == [a[1]] * 3, (what, a[1:4], b[1:4])
        if i < len(want):
            assert oracle == want[i], what
        assert b[4:8] == ["0"] * 4, (what, "a second pass with the knob at 0")
        assert a[4] == "0", (what, "the G chain from the identity can never be flagged")
        assert a[6] == "0", (what, "the key chain from the identity is not flagged by these inputs")
        assert _affine(a[8:13]) == _affine(b[8:13]), (what, "R_G")
        assert _affine(a[13:18]) == _affine(b[13:18]), (what, "R_Q")
        if a[5] == "1":
            redo_q.add(i)
        if a[7] == "1":
            redo_gf.add(i)
    crafted = {i for i, k in enumerate(kinds) if k[0] == "crafted"}
    golden_accepts = {i for i, k in enumerate(kinds) if k[0] == "golden" and k[1]["status"] == 1}
    assert crafted <= redo_q, sorted(crafted - redo_q)
    assert not (redo_q | redo_gf) & golden_accepts
    # the golden group-law tags are what the second pass is for
    by_tag = {}
    for i in redo_q | redo_gf:
        if kinds[i][0] == "golden":
            by_tag[kinds[i][1]["tag"]] = by_tag.get(kinds[i][1]["tag"], 0) + 1
    print("second pass: device order", len(redo_q), "host order", len(redo_gf), "golden tags", by_tag)
    # r_inf ends on P + (-P) in its last addition; r_double (u1 G == u2 Q) doubles only in an
    # addition of the two whole sums, which a windowed chain never forms
    assert by_tag.get("r_inf", 0) > 0
    assert set(by_tag) <= {"r_inf", "r_double", "small_key"}, by_tag
    # everything else in the device order's set is an edge vector built to end on the identity or to double
    assert all(kinds[i][0] != "golden" or kinds[i][1]["tag"] in ("r_inf", "r_double", "small_key") for i in redo_q)


def test_sanitized_build(exes, inputs, tmp_path):
    """The crafted vectors and the golden group-law items through the
    AddressSanitizer + UBSan build (stand-alone executable)."""
    batch, kinds = inputs
    from babble_amd.batch import BatchBuilder

    bb = BatchBuilder()
    n = 0
    for i, k in enumerate(kinds):
        if k[0] == "crafted" or (k[0] == "golden" and k[1]["tag"] in ("r_inf", "r_double", "small_key", "valid")
                                 and i % 3 == 0):
            m0, m1 = int(batch.msg_off[batch.item_msg[i]]), int(batch.msg_off[batch.item_msg[i] + 1])
            k0, k1 = int(batch.key_off[batch.item_key[i]]), int(batch.key_off[batch.item_key[i] + 1])
            bb.add_item_raw(bb.add_msg(bytes(batch.msg_bytes[m0:m1])), bb.add_key(bytes(batch.key_bytes[k0:k1])),
                            int(batch.pre[i]), bytes(batch.r_be[i]), bytes(batch.s_be[i]))
            n += 1
    assert n >= 24
    out = _run(exes["asan"], bb.pack().as_dict(), tmp_path, "asan")
    assert len(out) == n
    assert all(t[1] == t[2] == t[3] for t in out)
    assert sum(t[5] == "1" for t in out) >= 24


def test_device_g_chain_is_never_flagged():
    """k_verify_g on the device entry (26-bit signed windows x 10, from the
    identity): before window j the partial sum is at most 2^25 (2^(26 j) - 1)
    / (2^26 - 1) < 2^(26 j) in magnitude, the entry is a nonzero multiple of
    2^(26 j), and
    the total is u1 in (0, N) — so the accumulator never equals the entry or
    its opposite, on any u1; asserted here on every edge vector's u1."""
    W, NWIN = 26, 10
    n = 0
    for v in ev.vectors():
        if not (0 < v.s < N and 0 < v.r < N):
            continue
        u1 = v.u1
        d = ev.signed_digits(u1, W, NWIN)
        assert sum(x << (W * j) for j, x in enumerate(d)) == u1
        part = 0
        for j, x in enumerate(d):
            entry = x << (W * j)
            if x and part:
                # |partial| <= 2^(W-1) (1 + 2^W + ... + 2^(W (j-1))) < 2^(W j) <= |entry|
                assert abs(part) * ((1 << W) - 1) <= (1 << (W - 1)) * ((1 << (W * j)) - 1) and abs(part) < abs(entry)
                assert (part - entry) % N and (part + entry) % N, (v.tag, j)
                n += 1
            part += entry
        assert 0 <= part < N
    assert n > 1000
