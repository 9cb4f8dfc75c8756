"""The trimmed last addition (point.h gexz_add_ge xz_only) and key_table_add
with the GLV half's sign folded into the entries' signs, against the full
forms and against Python integers (oracle.gosemantics curve code).

tests/finaladd/finaladd_main.cpp is a stand-alone host program compiled from
the device's own source under AddressSanitizer + UBSan (nothing is loaded into
Python); it is built twice, with the lookups one window ahead
(BV_LOOKUP_PIPE=3, the default) and without, and both run every case.  Its
key tables are 4-bit signed windows x 33, built here with integers.
"""
import os
import random
import subprocess

import pytest

from oracle import gosemantics as gs

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "finaladd")
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
P, N = gs.P, gs.N
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
TW, TN = 4, 33
ENT = 1 << (TW - 1)


def hx(v):
    return f"{v % P:064x}"


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def phi(pt):
    return None if pt is None else (BETA * pt[0] % P, pt[1])


def mul(k, pt):
    if k < 0:
        return neg(gs.scalar_mult(-k, pt))
    return gs.scalar_mult(k, pt) if k else None


def acc(pt, rng):
    """XYZZ accumulator line fields for an affine point (None: identity)."""
    if pt is None:
        return f"{hx(0)} {hx(0)} {hx(0)} {hx(0)} 1"
    z = rng.randrange(1, P)
    return f"{hx(pt[0] * z * z)} {hx(pt[1] * z ** 3)} {hx(z * z)} {hx(z ** 3)} 0"


def r_of(pt, accept):
    """An r that final_check accepts / rejects for the sum `pt`."""
    if pt is None:
        return hx(1)
    r = pt[0] % N
    return hx(r if accept else (r + 1) % N)


@pytest.fixture(scope="module")
def exes():
    out = {}
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    for pipe in (3, 0):
        exe = os.path.join(HERE, "_build", f"finaladd_pipe{pipe}")
        subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", f"-DBV_LOOKUP_PIPE={pipe}", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(HERE, "finaladd_main.cpp"), "-o", exe], check=True, cwd=ROOT)
        out[pipe] = exe
    return out


@pytest.fixture(scope="module")
def key():
    """A key Q and its two half-tables as 'T x y' lines: entry j * ENT + d =
    d 2^(W j) Q for 0 < d <= ENT (zeros at index 0), then the phi half."""
    rng = random.Random(5)
    q = gs.scalar_mult(rng.randrange(1, N), gs.G)
    ents = [None] * (TN * ENT + 1)
    for j in range(TN):
        for d in range(1, ENT + 1):
            ents[j * ENT + d] = gs.scalar_mult(d << (TW * j), q)
    lines = []
    for f in (lambda e: e, phi):
        for e in ents:
            e = f(e)
            lines.append("T " + (f"{hx(0)} {hx(0)}" if e is None else f"{hx(e[0])} {hx(e[1])}"))
    return q, lines


def run(exes, tmp_path, lines):
    """Run both builds over the case lines: [[tokens of case 0], ...] each."""
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    outs = []
    for pipe, exe in exes.items():
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600,
                           env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "PATH": "/usr/bin:/bin"})
        assert r.returncode == 0, (pipe, r.stdout[-2000:] + r.stderr[-4000:])
        outs.append([ln.split() for ln in r.stdout.splitlines()])
    assert outs[0] == outs[1], "the pipelined and the load-then-add loops differ"
    return outs[0]


def check(tok, want, accept, what, whole=False):
    """tok: new X ZZ inf dec | full X ZZ inf dec Y ZZZ [| new Y ZZZ]."""
    new, full = tok[0:4], tok[4:8]
    assert new == full, f"{what}: X, ZZ, identity flag or decision differ from the full form"
    inf, dec = int(full[2]), int(full[3])
    assert inf == (want is None), what
    assert dec == (1 if accept and want is not None else 0), what
    if want is not None:
        X, ZZ, Y, ZZZ = (int(t, 16) for t in (full[0], full[1], tok[8], tok[9]))
        assert X * pow(ZZ, -1, P) % P == want[0], what
        assert pow(ZZ, 3, P) == ZZZ * ZZZ % P, what
        if whole:  # the folded sign keeps the whole point, not only x
            Y, ZZZ = int(tok[10], 16), int(tok[11], 16)
        assert Y * pow(ZZZ, -1, P) % P == want[1], what


def test_trimmed_final_addition(exes, tmp_path):
    rng = random.Random(11)
    cases = []
    for _ in range(12):
        a, b = mul(rng.randrange(1, N), gs.G), mul(rng.randrange(1, N), gs.G)
        cases.append((a, b, "random"))
    a = mul(rng.randrange(1, N), gs.G)
    b = mul(rng.randrange(1, N), gs.G)
    cases += [(None, b, "identity accumulator"), (a, a, "doubling"), (a, neg(a), "identity result")]
    lines, wants = [], []
    for a, b, what in cases:
        want = gs.point_add(a, b)
        for accept in (True, False):
            lines.append(f"add {acc(a, rng)} {hx(b[0])} {hx(b[1])} {r_of(want, accept)}")
            wants.append((want, accept, what))
    out = run(exes, tmp_path, lines)
    assert len(out) == len(wants)
    for tok, (want, accept, what) in zip(out, wants):
        check(tok, want, accept, what)


K_CASES = [("zero", 0), ("one", 1), ("all ones: every carry, top digit 1", (1 << 128) - 1),
           ("top digit 0", (1 << 123) + 12345), ("digit 2^W/2 and above", 0x89898989898989898989898989898989)]


def test_sign_folded_half(exes, key, tmp_path):
    q, table = key
    rng = random.Random(12)
    ks = K_CASES + [(f"random {i}", rng.randrange(1 << 128)) for i in range(6)]
    lines, wants = [], []
    for what, k in ks:
        for ng in (0, 1):
            for ph in (0, 1):
                base = phi(q) if ph else q
                term = mul(-k if ng else k, base)
                starts = [("random acc", mul(rng.randrange(1, N), gs.G), 0), ("identity acc", None, 0),
                          ("identity acc, from_inf", None, 1), ("sum is the identity", neg(term), 0)]
                if k == (1 << 128) - 1:  # the top window's entry equals the running sum: a doubling
                    starts.append(("last addition doubles", mul(-((1 << 129) - k) if ng else (1 << 129) - k, base), 0))
                for sw, a, from_inf in starts:
                    want = gs.point_add(a, term)
                    for last in (0, 1):
                        lines.append(f"half {acc(a, rng)} {k:064x} {ng} {ph} {from_inf} {last} {r_of(want, True)}")
                        wants.append((want, f"{what}, neg {ng}, phi {ph}, {sw}, last {last}", not last))
    out = run(exes, tmp_path, table + lines)
    assert len(out) == len(wants)
    for tok, (want, what, whole) in zip(out, wants):
        check(tok, want, True, what, whole)


def test_two_halves_and_decision(exes, key, tmp_path):
    """verify_item_q's loop: R_G + k1 Q + k2 phi(Q) for both signs of both
    halves, stored phi half (K12) and phi per lookup (KC), empty halves."""
    q, table = key
    rng = random.Random(13)
    lines, wants = [], []
    pairs = [(rng.randrange(1 << 128), rng.randrange(1 << 128)) for _ in range(3)]
    pairs += [(0, rng.randrange(1 << 128)), (rng.randrange(1 << 128), 0), (0, 0), ((1 << 128) - 1, (1 << 128) - 1)]
    for k1, k2 in pairs:
        for signs in range(4):
            for kc in (0, 1):
                t = gs.point_add(mul(-k1 if signs & 1 else k1, q), mul(-k2 if signs & 2 else k2, phi(q)))
                for sw, rg in (("random R_G", mul(rng.randrange(1, N), gs.G)), ("identity R_G", None),
                               ("sum is the identity", neg(t))):
                    want = gs.point_add(rg, t)
                    for accept in (True, False):
                        lines.append(f"item {acc(rg, rng)} {k1:064x} {k2:064x} {signs} {kc} {r_of(want, accept)}")
                        wants.append((want, accept, f"k1 {k1:x} k2 {k2:x} signs {signs} kc {kc}, {sw}"))
    out = run(exes, tmp_path, table + lines)
    assert len(out) == len(wants)
    for tok, (want, accept, what) in zip(out, wants):
        check(tok, want, accept, what)
