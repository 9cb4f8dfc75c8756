"""k_sinv's block-level batch inversion (verify_core.h BV_SINV_BLOCK:
sinv_lane_prefix, sinv_block_lane, sinv_lane_finish) against the parent's one
inversion per lane (sinv_thread), word for word, and against Python integers.

tests/sinvblock/sinvblock_main.cpp is a stand-alone host program compiled from
the device's own source (nothing is loaded into Python), once plainly and once
with -fsanitize=address,undefined; it replays both kernels lane by lane with
the launcher's geometry over buffers of exactly n items.

Every case mixes in the items k_sinv must step over (s = 0, s >= N, pre != 0):
first and last in a lane, alone in a lane, a whole lane of them, and for the
larger batches a whole block of them.
"""
import os
import random
import subprocess

import pytest

from oracle import gosemantics as gs

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sinvblock")
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
N = gs.N
R = 1 << 256
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 4099]
MS = [1, 2, 3, 16]
BLOCK = 256  # the launcher's block, and that of the per-lane kernel


def geometry(n, m, block=BLOCK):
    threads = -(-n // m)
    return -(-threads // block) * block  # T: item i is lane i % T's item i // T


def make_case(n, m):
    """[(s, pre)] and the set of unusable indices."""
    rng = random.Random(0x51B0 + 131 * n + m)
    T = geometry(n, m)
    items = [(rng.randrange(1, N), 0) for _ in range(n)]
    kinds = [lambda: (0, 0), lambda: (N, 0), lambda: (N + 1 + rng.randrange(R - N - 1), 0), lambda: (R - 1, 0),
             lambda: (rng.randrange(1, N), 1), lambda: (rng.randrange(1, N), 0x80)]
    bad = set()

    def spoil(i):
        if 0 <= i < n and i not in bad:
            items[i] = kinds[len(bad) % len(kinds)]()
            bad.add(i)

    lanes = {}
    for i in range(n):
        lanes.setdefault(i % T, []).append(i)
    order = sorted(lanes)
    pick = lambda frac: order[min(len(order) - 1, int(frac * len(order)))]
    spoil(lanes[pick(0.0)][0])  # first in its lane (and the batch's first item)
    spoil(lanes[pick(0.3)][-1])  # last in its lane
    spoil(lanes[pick(0.55)][0])
    spoil(n - 1)  # the batch's last item
    for i in lanes[pick(0.8)]:  # a whole lane
        spoil(i)
    alone = [t for t in order if len(lanes[t]) == 1]
    if alone:
        spoil(lanes[alone[len(alone) // 2]][0])  # alone in its lane
    if n == 4099:  # the whole second block
        for i in range(n):
            if BLOCK <= i % T < 2 * BLOCK:
                spoil(i)
    return items, bad


CASES = {(n, m): make_case(n, m) for n in SIZES for m in MS}


def test_cases_cover_the_special_items():
    assert all(bad for _, bad in CASES.values())
    items, bad = CASES[(4099, 2)]
    T = geometry(4099, 2)
    assert T > 2 * BLOCK and {i for i in range(4099) if BLOCK <= i % T < 2 * BLOCK} <= bad
    assert any(s == 0 for s, _ in items) and any(s >= N for s, _ in items) and any(p for _, p in items)
    assert len(bad) < 4099 // 2


def build(name, extra):
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    exe = os.path.join(HERE, "_build", name)
    subprocess.run([CLANGXX, "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
                   + extra + [os.path.join(HERE, "sinvblock_main.cpp"), "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("sinvblock") / "cases.txt")
    with open(path, "w") as f:
        for (n, m), (items, _) in CASES.items():
            f.write(f"CASE {n} {m}\n")
            for s, pre in items:
                f.write(f"{s:064x} {pre}\n")
    return path


def run(exe, block, cases_file):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(block), cases_file], capture_output=True, text=True, timeout=600, env=env)
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[0] == "CASE":
            cur = (int(f[1]), int(f[2]))
            out[cur] = dict(usable=int(f[3]), differ=int(f[4]), w={})
        else:
            out[cur]["w"][int(f[1])] = int(f[2], 16)
    return r.returncode, out, r.stderr


@pytest.fixture(scope="module", params=["plain", "sanitized", "plain-1024", "plain-64"])
def result(request, cases_file):
    if request.param == "sanitized":
        exe = build("sinvblock_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      "-fno-omit-frame-pointer"])
    else:
        exe = build("sinvblock", [])
    block = int(request.param.split("-")[1]) if "-" in request.param else BLOCK
    return run(exe, block, cases_file)


def test_w_is_word_for_word_the_per_lane_form(result):
    rc, out, err = result
    assert rc == 0, err[-2000:]
    assert sorted(out) == sorted(CASES)
    for key, (items, bad) in CASES.items():
        assert out[key]["usable"] == len(items) - len(bad), key
        assert out[key]["differ"] == 0, key


def test_w_times_s_is_the_montgomery_one(result):
    rc, out, err = result
    assert rc == 0, err[-2000:]
    for key, (items, bad) in CASES.items():
        w = out[key]["w"]
        assert sorted(w) == [i for i in range(len(items)) if i not in bad], key
        for i, wi in w.items():
            assert wi < N and wi * items[i][0] % N == R % N, (key, i)
