"""The GLV split in plain integers (field.h glv_split_int, BV_GLV_INT) against
the earlier form (glv_split_mont: residues mod N through three Montgomery
products) and against Python integers.

tests/glvint/glvint_main.cpp is a stand-alone host program compiled from the
device's own source (nothing is loaded into Python).  It runs both forms side
by side on every scalar and fails on the first difference; it is built plain,
a second time under AddressSanitizer + UBSan, and a third time with
BV_GLV_INT=0 (the knob's other side selects the earlier form).  Python then
checks what the split must satisfy on its own: k1 + k2 lambda = k (mod N),
both magnitudes below 2^128, and equality with edge_vectors.glv_halves.
"""
import os
import random
import subprocess

import pytest

from tests import edge_vectors as ev

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "glvint")
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
N, LAM = ev.N, ev.LAMBDA
A1, B1, A2, B2 = ev._A1, ev._B1, ev._A2, ev._B2
G1, G2 = ev._G1, ev._G2
NRANDOM = 200_000


def limbs(words):
    return sum(w << (32 * i) for i, w in enumerate(words))


def field_h_constants():
    """The uint32 arrays of field.h by name."""
    import re

    text = open(os.path.join(ROOT, "babble_amd", "csrc", "field.h")).read()
    out = {}
    for m in re.finditer(r"static constexpr uint32_t (\w+)\[\d+\] = \{([^}]*)\}", text):
        out[m.group(1)] = limbs([int(w.strip().rstrip("u"), 16) for w in m.group(2).split(",")])
    return out


def test_constants_follow_from_the_existing_ones():
    c = field_h_constants()
    rinv = pow(1 << 256, -1, N)
    mb1, mb2, lam = c["GLV_MB1R"] * rinv % N, c["GLV_MB2R"] * rinv % N, c["GLV_LAMR"] * rinv % N
    assert lam == LAM and mb1 == -B1 and mb2 == N - B2
    a1, a2 = mb1 * lam % N, (N - mb2) * (N - lam) % N  # a_i = -b_i lambda (mod N)
    assert (a1, a2) == (A1, A2)
    assert (a1 + B1 * lam) % N == 0 and (a2 + B2 * lam) % N == 0
    assert B2 == A1
    m = 1 << 160
    assert c["GLV_NB1"] == -B1 and c["GLV_NA1"] == -a1 % m and c["GLV_NA2"] == -a2 % m
    assert c["GLV_G1"] == G1 and c["GLV_G2"] == G2


def scalars():
    rng = random.Random(0x61F)
    ks = [0, 1, N - 1, (N + 1) // 2, (N - 1) // 2, LAM, N - LAM]
    # one half zero, one half changing sign: k = k1 + k2 lambda for small halves
    for t in (1, 2, 3, rng.getrandbits(64), rng.getrandbits(126), (1 << 127) - 1, 1 << 127):
        for k1, k2 in ((t, 0), (-t, 0), (0, t), (0, -t), (1, t), (-1, t), (1, -t), (-1, -t), (t, 1), (t, -1),
                       (-t, 1), (-t, -1)):
            ks.append((k1 + k2 * LAM) % N)
    # halves next to the half-multiples of the lattice vectors: where the
    # nearest lattice point, so the sign and size of a half, changes
    for m1 in (-1, 0, 1):
        for m2 in (-1, 0, 1):
            c1, c2 = (m1 * A1 + m2 * A2) // 2, (m1 * B1 + m2 * B2) // 2
            for d1 in range(-2, 3):
                for d2 in range(-2, 3):
                    ks.append((c1 + d1 + (c2 + d2) * LAM) % N)
    # multiples of the vectors themselves are 0 mod N; next to them
    for m in (1, 2, 1 << 60):
        for d in range(-2, 3):
            ks.append((m * (A1 + B1 * LAM) + d) % N)
            ks.append((m * (A2 + B2 * LAM) + d * LAM) % N)
    # where the rounding bit (bit 383) of k g1 / k g2 flips
    for g in (G1, G2):
        top = (N * g) >> 384
        for m in [0, 1, 2, top - 1, top - 2] + [rng.randrange(top) for _ in range(40)]:
            k0 = -(-((m << 384) + (1 << 383)) // g)  # the first k with bit 383 of the low part set
            k1 = -(-((m + 1) << 384) // g)           # the first k past it
            for base in (k0, k1):
                for d in range(-2, 3):
                    if 0 <= base + d < N:
                        ks.append(base + d)
    ks += [v.u2 for v in ev.vectors()]
    ks += [rng.randrange(N) for _ in range(NRANDOM)]
    return ks


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    ks = scalars()
    path = str(tmp_path_factory.mktemp("glvint") / "scalars.txt")
    with open(path, "w") as f:
        f.write("".join(f"{k:064x}\n" for k in ks))
    return ks, path


def build(name, extra):
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    exe = os.path.join(HERE, "_build", name)
    subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + extra +
                   [os.path.join(HERE, "glvint_main.cpp"), "-o", exe], check=True, cwd=ROOT)
    return exe


def run(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-4000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def plain(case_file):
    """The plain build's output lines (it exits non-zero where the two forms differ)."""
    return run(build("glvint", ["-O2"]), case_file[1])


def test_old_and_new_agree_and_split_is_exact(case_file, plain):
    ks, out = case_file[0], plain
    assert len(out) == len(ks)
    for k, ln in zip(ks, out):
        m1, m2, signs = ln.split()
        m1, m2, signs = int(m1, 16), int(m2, 16), int(signs)
        k1, k2 = (-m1 if signs & 1 else m1), (-m2 if signs & 2 else m2)
        assert m1 < 1 << 128 and m2 < 1 << 128 and signs < 4
        assert (k1 + k2 * LAM) % N == k, hex(k)
        assert not (m1 == 0 and signs & 1) and not (m2 == 0 and signs & 2), hex(k)
        assert (k1, k2) == ev.glv_halves(k), hex(k)
    # the chosen scalars do what they are for: both signs of both halves, and empty halves
    seen = {(ln.split()[2], ln.split()[0].strip("0") == "", ln.split()[1].strip("0") == "") for ln in out[:1000]}
    assert {s for s, _, _ in seen} == {"0", "1", "2", "3"}
    assert any(z1 for _, z1, _ in seen) and any(z2 for _, _, z2 in seen)


def test_sanitized_build(case_file, plain):
    san = run(build("glvint_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                   "-fno-omit-frame-pointer"]), case_file[1])
    assert san == plain


def test_knob_zero_selects_the_earlier_form(case_file, plain):
    assert run(build("glvint_knob0", ["-O2", "-DBV_GLV_INT=0"]), case_file[1]) == plain
