"""The host entries' staging planner (babble_amd/csrc/hoststage.cpp) and the
host helpers the drivers share (hostdag.cpp: bv_dag_levels, the event-field
checker), CPU only: a stand-alone driver built with ASan + UBSan
(tests/hostfuzz_stage, run as a subprocess) carries every planned command out
with memcpy over exactly-sized buffers.

The literal cases are what the drivers enqueued before the planner existed,
worked out by hand from that code for one layout: five arrays of 0, 1, 255, 256
and 70 000 bytes, each with a 64-byte pad, in pieces of 4096 bytes.  The
layout (offset, bytes): (0, 0) (256, 1) (512, 255) (1024, 256) (1536, 70000),
71 680 bytes in all.  Commands: D<off>:<array>+<source offset>:<n> is a DMA from
caller memory, C... a pool copy into the staging block, S<off>:<n> a DMA from
the staging block."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostfuzz_stage")
EXE = os.path.join(HERE, "_build", "hostfuzz_stage")

SIZES = (0, 1, 255, 256, 70000)
SMALL_COPIES = ["C256:1+0:1", "C512:2+0:255", "C1024:3+0:256"]


def _layout(direct):
    return f"{len(SIZES)} " + " ".join(f"{n} 64 {int(i in direct)}" for i, n in enumerate(SIZES))


# (merge_runs, a0, a1, direct arrays) -> the commands, in order
LITERAL = {
    # bv_host_launch / bv_events_launch / bv_verify_blocks: piece by piece
    "pieces_none_direct": ((0, 0, 9000, ()), SMALL_COPIES + ["C1536:4+0:2560", "S0:4096",
                                                             "C4096:4+2560:4096", "S4096:4096",
                                                             "C8192:4+6656:808", "S8192:808"]),
    "pieces_big_direct": ((0, 0, 9000, (4,)), ["D1536:4+0:2560"] + SMALL_COPIES + ["S256:1", "S512:255", "S1024:256",
                                                                                 "D4096:4+2560:4096",
                                                                                 "D8192:4+6656:808"]),
    "pieces_all_direct": ((0, 0, 9000, (0, 1, 2, 3, 4)), ["D256:1+0:1", "D512:2+0:255", "D1024:3+0:256",
                                                          "D1536:4+0:2560", "D4096:4+2560:4096", "D8192:4+6656:808"]),
    # [a0, a1) begins and ends inside the 70 000-byte array: the pieces are counted from a0
    "pieces_inside_one_array": ((0, 2000, 10000, ()), ["C2000:4+464:4096", "S2000:4096",
                                                       "C6096:4+4560:3904", "S6096:3904"]),
    "pieces_inside_one_array_direct": ((0, 2000, 10000, (4,)), ["D2000:4+464:4096", "D6096:4+4560:3904"]),
    # the whole layout: 17 full pieces and one of 2048 bytes, of which the array fills 1904
    "pieces_whole_layout": ((0, 0, 71680, ()), SMALL_COPIES + ["C1536:4+0:2560", "S0:4096"] + [
        t for k in range(1, 17) for t in (f"C{4096 * k}:4+{4096 * k - 1536}:4096", f"S{4096 * k}:4096")
    ] + ["C69632:4+68096:1904", "S69632:2048"]),
    # the ITX / fields driver: the pool copies, then the copies in layout order, staged runs in one copy each
    "merge_none_direct": ((1, 0, 9000, ()), SMALL_COPIES + ["C1536:4+0:2560", "S0:4096",
                                                            "C4096:4+2560:4096", "S4096:4096",
                                                            "C8192:4+6656:808", "S8192:808"]),
    "merge_big_direct": ((1, 0, 9000, (4,)), SMALL_COPIES + ["S0:1536", "D1536:4+0:2560",
                                                             "D4096:4+2560:4096", "D8192:4+6656:808"]),
    # (a run between two direct arrays carries the first one's pad)
    "merge_all_direct": ((1, 0, 9000, (0, 1, 2, 3, 4)), ["S0:256", "D256:1+0:1", "S257:255", "D512:2+0:255",
                                                         "S767:257", "D1024:3+0:256", "S1280:256", "D1536:4+0:2560",
                                                         "D4096:4+2560:4096", "D8192:4+6656:808"]),
    "merge_inside_one_array": ((1, 2000, 10000, ()), ["C2000:4+464:4096", "S2000:4096",
                                                      "C6096:4+4560:3904", "S6096:3904"]),
}


@pytest.fixture(scope="module")
def driver():
    subprocess.run(["make", "-s", "-C", HERE], check=True)

    def run(lines):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
        out = p.stdout.splitlines()
        assert len(out) == len(lines), p.stdout[-3000:]
        return out

    return run


def test_range_plan_literal_cases(driver):
    names = list(LITERAL)
    out = driver([f"R {m} 4096 {a0} {a1} {_layout(direct)}" for (m, a0, a1, direct), _ in LITERAL.values()])
    for name, line in zip(names, out):
        f = line.split()
        assert f[:2] == ["R", "71680"], (name, line)
        assert f[2:] == LITERAL[name][1], name  # (a property that failed would add "FAIL ...")


def test_direct_floor_per_policy(driver):
    """mark_direct with every array in pinned memory: an empty array never goes
    direct; the fields driver's floor is 256 KiB; the ITX entry stages all."""
    sizes = "0 1 255 256 70000 262143 262144 300000"
    out = driver([f"M 0 {sizes}", f"M 262144 {sizes}", f"M -1 {sizes}"])
    assert out == ["M 01111111", "M 00000011", "M 00000000"]


def test_range_plan_properties(driver):
    """4,000 random layouts (empty and absent arrays, pads, direct and sliced
    arrays), piece sizes and ranges cut at phase ends or anywhere, both
    policies: every byte of every whole array inside the range reaches its
    device offset exactly once and from the right source (through the staging
    block exactly once unless direct); no command leaves the range or the
    layout; one staged DMA per piece when nothing in it is direct; as many
    DMAs as (array, piece) intersections when something is, piece by piece;
    no two staged DMAs of a piece adjacent under the merging policy (runs of
    different pieces meet at the piece boundary by construction); and the
    order within a piece."""
    assert driver(["F 20260101 4000"]) == ["F ok 4000"]


def test_slice_plan_chunks_tile_every_array(driver):
    """600 events in chunks of 256 and 200 in chunks of 64 (the last chunk of
    8), whole and as the shard [192, 792) of 900 / [64, 264) of 300 with every
    base non-zero; with and without transactions, with and without the fragment
    arrays; no event at a chunk edge has a transaction.  Per array the chunks'
    byte ranges start at 0, end at its length and follow one another without
    gap or overlap but the one shared element of an n + 1 offset array, and the
    commands carried out leave the array's bytes at its device offset."""
    assert driver(["L"]) == ["L ok 48"]


def test_dag_levels_equal_restatement(driver):
    assert driver(["G"]) == ["G ok 6"]


def test_event_field_checker_same_verdict_with_and_without_pool(driver):
    """300 000 events (three grains), one thing wrong near the end: the pool's
    scan and the caller's give the same verdict, for the verify entries' rules
    and for the context-free helpers' (which do not read the signatures)."""
    f = driver(["V"])[0].split()
    assert f[0] == "V" and len(f) == 1 + 3 * 2 * 19
    ok = {"valid", "valid_again", "backward_reference"}
    seen = set()
    for name, alone, pooled in zip(f[1::3], f[2::3], f[3::3]):
        assert alone == pooled, name
        assert alone == ("0" if name.split("/")[0] in ok or name == "null_s/helper" else "1"), name
        seen.add(name)
    assert {"forward_reference", "forward_reference/helper", "tx_off_order", "fragment_order"} <= seen
