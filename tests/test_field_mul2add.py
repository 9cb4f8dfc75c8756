"""fe_mul2add (r = a b + x y mod p with one Comba pass and one fold): the
generated gfx950 program executed by the generator's interpreter, and the
host form of babble_amd/csrc/field.h (a stand-alone program under
AddressSanitizer + UBSan; nothing is loaded into Python), against Python
integers over the operand classes of tests/mul2add_vectors.py.  The
interpreter asserts the program's bounds while it runs (the carry-outs the
program claims are zero: R_9 <= 2, the second fold's limbs 1..2), and the
test asserts that each rare block was in fact entered."""
import os
import subprocess
import sys

import pytest

from tests import mul2add_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "mul2add")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_field_asm as G  # noqa: E402

P = V.P
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")


@pytest.fixture(scope="module")
def cases():
    return V.classes(300, seed=1)


def _run(g, q, force_slow=False):
    m = G.Machine()
    for name, val in zip("abxy", q):
        for i in range(8):
            m.r[f"%[{name}{i}]"] = (val >> (32 * i)) & G.M32
    m.run(g, force_slow)
    return sum(m.r[f"%[r{i}]"] << (32 * i) for i in range(8)), m.hits


@pytest.mark.parametrize("force_slow", [False, True])
def test_interpreter_matches_python_ints(cases, force_slow):
    """force_slow runs every rare block for every operand: each must be a
    no-op for lanes that did not ask for it."""
    g = G.build("fe_mul2add")
    hits = {}
    for cls, qs in cases.items():
        for q in qs:
            r, h = _run(g, q, force_slow)
            a, b, x, y = q
            assert r < 2**256 and (r - (a * b + x * y)) % P == 0, (cls, [hex(v) for v in q], hex(r))
            for k, n in h.items():
                hits[cls, k] = hits.get((cls, k), 0) + n
    # each class drives the block it is named for
    assert hits["recount", "fe_mul2add_recount"] > 0
    assert hits["ycarry", "fe_mul2add_ycarry"] > 100
    assert hits["tail", "fe_mul2add_tail"] == len(cases["tail"])
    assert hits["random", "fe_mul2add_recount"] == 0 and hits["random", "fe_mul2add_tail"] == 0
    assert all(a * b + x * y >= 2**512 for a, b, x, y in cases["limb17"]) and len(cases["limb17"]) > 50


def test_second_wrap_of_the_tail(cases):
    """Half of the tail class also carries out of limb 7 inside the tail:
    the value left is below 2^67 and takes 2^32 + 977 once more."""
    n = 0
    for a, b, x, y in cases["tail"]:
        s = a * b + x * y
        f = s % 2**256 + V.K * (s >> 256)          # first fold
        n += f % 2**256 + V.K * (f >> 256) >= 2**256
    assert n >= len(cases["tail"]) // 2


def test_program_shape():
    g = G.build("fe_mul2add")
    G.check_hazards(g)
    assert G.outputs_after_inputs(g)             # outputs need no early-clobber
    st = G.stats(g)
    assert st["mad"] + st["mad_nc"] == 128 + 8 + 2   # both products, the fold, the second fold
    valu = sum(v for k, v in st.items() if k not in ("nop", "sor", "rare_mid", "rare_tail"))
    mul = G.stats(G.build("fe_mul"))
    sub = G.stats(G.build("fe_sub"))
    count = lambda d: sum(v for k, v in d.items() if k not in ("nop", "sor", "rare_mid", "rare_tail"))
    # against two products and a subtraction, and still with the negation it needs
    assert valu + count(sub) < 2 * count(mul) + count(sub) - 25


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    out = os.path.join(HERE, "_build", "mul2add_host")
    subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "mul2add_main.cpp"), "-o", out], check=True, cwd=ROOT)
    return out


def test_host_form_matches_python_ints(cases, exe, tmp_path):
    qs = [q for c in cases.values() for q in c]
    path = str(tmp_path / "ops.txt")
    with open(path, "w") as f:
        for q in qs:
            f.write(" ".join(f"{v:064x}" for v in q) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [int(ln, 16) for ln in r.stdout.split()]
    assert len(out) == len(qs)
    bad = [(hex(a), hex(b), hex(x), hex(y), hex(z)) for (a, b, x, y), z in zip(qs, out)
           if z >= 2**256 or (z - (a * b + x * y)) % P]
    assert not bad, bad[:3]
