"""The table-audit relations (tests/tablecheck/audit.h) against themselves on
the CPU: a clean table passes, every corruption class is caught, and only by
the relations that read the touched slots.

tests/tablecheck/audit_main.cpp is a stand-alone host program (nothing is
loaded into Python).  It builds one K8 and one K12 table for two keys by plain
per-entry double-and-add, audits them serially with the same functions the
device kernels of tests/tablecheck/tablecheck.hip call, then audits copies
with one corruption each.  It runs twice: plain, and built with
-fsanitize=address,undefined.
"""
import os
import random
import subprocess

import pytest

from oracle import gosemantics as gs

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tablecheck")
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
R0, R1, R2, R3, R4 = range(5)
# required entries, both halves, two keys (the issue's counts per half)
AUDITED = {"K8": 2 * 2 * 16 * 255, "K12": 2 * 2 * (10 * 2 ** 11 + 2 ** 8)}
SLOT = {"K8": (7, 100, 255), "K12": (5, 1000, 2048)}  # window, digit, the window's top digit


def keys():
    rng = random.Random(0x7AB1E)
    return [gs.G, gs.scalar_mult(rng.randrange(1, gs.N), gs.G)]


def expected(table, name):
    """The failures (relation, key, window, digit) each case must report: the
    relations that read a touched slot, and no other."""
    j, d, top = SLOT[table]
    e = {
        "clean": [],
        # the plain entry alone changes: its own step, the next step, its phi entry
        "flipx": [(R1, 0, j, d), (R1, 0, j, d + 1), (R4, 0, j, d)],
        "negy": [(R1, 0, j, d), (R1, 0, j, d + 1), (R4, 0, j, d)],
        # both halves move together: only the steps see it
        "swap": [(R1, 0, j, d), (R1, 0, j, d + 1), (R1, 0, j, d + 2)],
        "nextwin": [(R1, 0, j, d), (R1, 0, j, d + 1)],
        "phix": [(R4, 0, j, d)],
        "zeroed": [(R1, 0, j, d), (R1, 0, j, d + 1), (R3, 0, j, d), (R4, 0, j, d)],
        "noncanon": [(R1, 0, j, d), (R1, 0, j, d + 1), (R3, 0, j, d), (R4, 0, j, d)],
        "flipx_top": [(R1, 0, j, top), (R2, 0, j + 1, 1), (R4, 0, j, top)],
        # T[0][1] is also B of every step of window 0 from d = 3 on, and A of d = 2
        "anchor": None,
    }
    return e[name]


def build(san):
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    exe = os.path.join(HERE, "_build", "audit_asan" if san else "audit")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
    subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(HERE, "audit_main.cpp"), "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def result(request, tmp_path_factory):
    exe = build(request.param)
    path = str(tmp_path_factory.mktemp("tablecheck") / "keys.txt")
    with open(path, "w") as f:
        for x, y in keys():
            f.write(f"{x:064x} {y:064x}\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    cases, forms = {}, {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "CASE":
            cases[(w[1], w[2])] = (int(w[3]), int(w[4]), [tuple(int(v) for v in t.split(":")) for t in w[5:]])
        elif w[0] == "FORM":
            forms[w[1]] = int(w[2])
    return cases, forms


def test_clean_tables_pass_and_every_required_entry_is_audited(result):
    cases, _ = result
    for table in ("K8", "K12"):
        audited, n, fails = cases[(table, "clean")]
        assert (n, fails) == (0, []), (table, fails)
        assert audited == AUDITED[table]


@pytest.mark.parametrize("table", ["K8", "K12"])
@pytest.mark.parametrize("name", ["flipx", "negy", "swap", "nextwin", "phix", "zeroed", "noncanon"])
def test_corruption_is_caught_where_it_is_read(result, table, name):
    cases, _ = result
    audited, n, fails = cases[(table, name)]
    assert audited == AUDITED[table]
    assert n == len(fails) and fails == sorted(expected(table, name)), (table, name, fails)
    assert all(f[1] == 0 for f in fails), "the untouched key reported a failure"


def test_top_digit_in_next_windows_slot_zero(result):
    cases, _ = result
    assert ("K8", "flipx_top") not in cases  # unsigned: no such slot
    _, n, fails = cases[("K12", "flipx_top")]
    assert n == 3 and fails == sorted(expected("K12", "flipx_top")), fails


def test_k8_slot_zero_is_the_identity_in_both_halves(result):
    cases, _ = result
    assert ("K12", "slot0") not in cases  # signed: slot 0 holds the window below's top digit
    _, n, fails = cases[("K8", "slot0")]
    assert n == 1 and fails == [(R3, 0, SLOT["K8"][0], 0)], fails


@pytest.mark.parametrize("table", ["K8", "K12"])
def test_anchor(result, table):
    """T[0][1] changed (y bit 0): R0 sees it; so do its phi entry and every
    step of window 0 (it is B of each of them), and nothing outside window 0
    but the link into window 1 of K8, which adds T[0][1]."""
    cases, _ = result
    j, d, top = SLOT[table]
    _, n, fails = cases[(table, "anchor")]
    assert (R0, 0, 0, 1) in fails and (R4, 0, 0, 1) in fails and (R1, 0, 0, 2) in fails
    assert n == 2 + (top - 1) + (1 if table == "K8" else 0)
    assert all(f[1] == 0 and (f[2] == 0 or f == (R2, 0, 1, 1)) for f in fails)


def test_form(result):
    _, forms = result
    assert forms == {"small": 1, "x_plus_p": 0, "y_plus_p": 0, "zero": 0, "x_is_p": 0}
