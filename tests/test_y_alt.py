"""BV_Y_ALT (the verify additions store S and -S in turn: no negation for the
fused Y3) on the CPU.

tests/yalt/yalt_main.cpp compiles verify_core.h for the host (through the host
emulator's table builders) as a stand-alone program with the knob at 1 and at
0, and once under AddressSanitizer + UBSan; nothing is loaded into Python.
Over the golden items, the chosen-scalar edge vectors, the crafted doubling
and inverse vectors of tests/defer_vectors.py and the zero-window vectors of
tests/yalt_vectors.py both builds must give, item for item, the C oracle's
status in the device entry's order (verify_item_g, then verify_item_q) and in
the host entries' order (verify_item_qfirst, then verify_item_gfinish), and
stored partial sums R_G / R_Q that are the same group elements.  The host
emulator's generator geometry has 17 windows and K12 has 11 a half, both odd,
so every chain also ends in the negated state and is put back (y_true).

The program counts the entries into the rare paths of the addition steps; the
crafted set must reach each of them: the skip fix-up (a zero digit), the
identity taking an entry, the doubling and P + (-P).
"""
import os
import subprocess

import pytest

from tests import defer_vectors as dv
from tests import edge_vectors as ev
from tests import yalt_vectors as yv
from tests.emu import emu
from tests.helpers import golden_items_batch, load

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "yalt")
ROOT = os.path.dirname(os.path.dirname(HERE))
BUILD = os.path.join(HERE, "_build")
LLVM = os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin")
P, N = ev.P, ev.N
# the emulator's 16-bit generator geometry (a 64 MB table)
GW, GNWIN = 16, 17
GEOM = [f"-DBV_GW={GW}", f"-DBV_GNWIN={GNWIN}", "-DBV_GL=8", "-DBV_GNSUB=34"]
CSRC = os.path.join(ROOT, "babble_amd", "csrc")
ACCEPT = 1


def _build(name, knobs, extra):
    os.makedirs(os.path.join(BUILD, name), exist_ok=True)
    flags = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + GEOM + knobs + extra
    objs = []
    for src, lang, std in ((os.path.join(HERE, "yalt_main.cpp"), "c++", "-std=c++17"),
                           (os.path.join(CSRC, "hostsha.cpp"), "c++", "-std=c++17"),
                           (os.path.join(CSRC, "hostdag.cpp"), "c++", "-std=c++17"),
                           (os.path.join(ROOT, "oracle", "oracle.c"), "c", "-std=c11")):
        obj = os.path.join(BUILD, name, os.path.basename(src) + ".o")
        cc = os.path.join(LLVM, "clang++" if lang == "c++" else "clang")
        subprocess.run([cc, "-x", lang, std] + flags + ["-c", src, "-o", obj], check=True, cwd=ROOT)
        objs.append(obj)
    exe = os.path.join(BUILD, name, "yalt")
    subprocess.run([os.path.join(LLVM, "clang++")] + extra + ["-o", exe] + objs + ["-lpthread"], check=True)
    return exe


@pytest.fixture(scope="module")
def exes():
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    return {"on": _build("on", ["-DBV_Y_ALT=1"], ["-O2"]),
            "off": _build("off", ["-DBV_Y_ALT=0"], ["-O2"]),
            "asan": _build("asan", ["-DBV_Y_ALT=1"], san)}


@pytest.fixture(scope="module")
def inputs():
    """(batch, kinds): kinds[i] is ('golden', item) / ('edge', Vector) /
    ('crafted', tag) / ('zero', tag) (an ACCEPT on a key of its own) /
    ('zero2', tag) (on a shared key) of item i."""
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
    for tag, body, pub, r, s in yv.vectors(GW, GNWIN):
        bb.add_item_raw(bb.add_msg(body), bb.add_key(pub), 0, r.to_bytes(32, "big"), s.to_bytes(32, "big"))
        kinds.append(("zero", tag))
    for tag, body, pub, r, s in yv.shared_key_vectors(GW, GNWIN):
        bb.add_item_raw(bb.add_msg(body), bb.add_key(pub), 0, r.to_bytes(32, "big"), s.to_bytes(32, "big"))
        kinds.append(("zero2", tag))
    return bb.pack(), kinds


def _run(exe, arrs, tmp_path, name, knob):
    path = str(tmp_path / f"{name}.bin")
    emu.dump_batch(path, arrs)
    r = subprocess.run([exe, path, "8"], capture_output=True, text=True, timeout=900,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, (name, r.stdout[-1000:] + r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0] == f"knob {knob}", lines[0]
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


def test_the_zero_window_vectors_are_what_they_claim():
    pats_g, pats_k = yv.patterns(GNWIN), yv.patterns(yv.KNWIN)
    seen = set()
    for tag, body, pub, r, s in yv.vectors(GW, GNWIN):
        _, _, which, name = tag.split("/")
        zu, z1, z2 = yv.zero_windows(body, r, s, GW, GNWIN)
        got, want = {"u1": (zu, pats_g), "h0": (z1, pats_k), "h1": (z2, pats_k)}[which]
        assert set(want[name]) <= set(got), (tag, got)
        seen.add((which, name))
    # window 0, an even and an odd window, two consecutive windows, the last window: u1 and both halves
    assert seen == {(w, n) for w in ("u1", "h0", "h1") for n in ("w0", "even", "odd", "pair", "last", "w0w1")}
    assert pats_k["even"][0] % 2 == 0 and pats_k["odd"][0] % 2 == 1
    assert pats_k["pair"][1] == pats_k["pair"][0] + 1 and pats_k["last"] == (yv.KNWIN - 1,)


def test_knob_on_and_off_agree_with_the_oracle(exes, inputs, tmp_path):
    batch, kinds = inputs
    on = _run(exes["on"], batch.as_dict(), tmp_path, "on", 1)
    off = _run(exes["off"], batch.as_dict(), tmp_path, "off", 0)
    assert len(on) == len(off) == len(kinds)
    _, expected, _ = golden_items_batch()
    want = list(expected) + list(ev.direct_statuses())
    counts = {k: [0, 0, 0, 0] for k in ("golden", "edge", "crafted", "zero", "zero2")}
    for i, (a, b) in enumerate(zip(on, off)):
        what = (i, kinds[i][0], kinds[i][1] if kinds[i][0] in ("crafted", "zero", "zero2") else getattr(kinds[i][1], "tag", ""))
        oracle = int(a[1])
        # both entry orders, both builds: the oracle's status
        assert a[1:4] == [a[1]] * 3 and b[1:4] == [a[1]] * 3, (what, a[1:4], b[1:4])
        if i < len(want):
            assert oracle == want[i], what
        if kinds[i][0] == "zero":
            assert oracle == ACCEPT, what
        # the rare paths are a property of the item, not of the knob
        assert a[4:8] == b[4:8], (what, a[4:8], b[4:8])
        assert _affine(a[8:13]) == _affine(b[8:13]), (what, "R_G")
        assert _affine(a[13:18]) == _affine(b[13:18]), (what, "R_Q")
        for k in range(4):
            counts[kinds[i][0]][k] += int(a[4 + k])
    print("skip / set / dbl / opp entries:", counts)
    crafted = [x + y for x, y in zip(counts["crafted"], counts["zero"])]
    assert all(c > 0 for c in crafted), crafted
    # every zero-window vector skips in both entry orders; the doubling and inverse vectors exit in the device order
    n_zero = sum(k[0] == "zero" for k in kinds)
    assert counts["zero"][0] >= 2 * n_zero
    # u1 and both halves at once: three chains an order, each skipping at least once
    assert counts["zero2"][0] >= 6 * sum(k[0] == "zero2" for k in kinds)
    assert counts["crafted"][2] >= 12 and counts["crafted"][3] >= 12


def test_sanitized_build(exes, inputs, tmp_path):
    """The crafted vectors, the zero-window vectors and a third of the golden
    group-law items through the AddressSanitizer + UBSan build (stand-alone
    executable)."""
    batch, kinds = inputs
    from babble_amd.batch import BatchBuilder

    bb = BatchBuilder()
    n = 0
    for i, k in enumerate(kinds):
        if k[0] in ("crafted", "zero", "zero2") or (k[0] == "golden" and i % 3 == 0
                                           and k[1]["tag"] in ("r_inf", "r_double", "small_key", "valid")):
            m0, m1 = int(batch.msg_off[batch.item_msg[i]]), int(batch.msg_off[batch.item_msg[i] + 1])
            k0, k1 = int(batch.key_off[batch.item_key[i]]), int(batch.key_off[batch.item_key[i] + 1])
            bb.add_item_raw(bb.add_msg(bytes(batch.msg_bytes[m0:m1])), bb.add_key(bytes(batch.key_bytes[k0:k1])),
                            int(batch.pre[i]), bytes(batch.r_be[i]), bytes(batch.s_be[i]))
            n += 1
    assert n >= 24 + 18
    out = _run(exes["asan"], bb.pack().as_dict(), tmp_path, "asan", 1)
    assert len(out) == n
    assert all(t[1] == t[2] == t[3] for t in out)
    assert sum(int(t[4]) > 0 for t in out) >= 18 and sum(int(t[6]) + int(t[7]) > 0 for t in out) >= 24
