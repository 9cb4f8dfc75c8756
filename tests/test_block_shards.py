"""bv_group_verify_blocks' host side, CPU only: the block-shard plan
(bv_plan_block_shards, csrc/hostplan.cpp) against its Python restatement
(babble_amd/shard.py plan_block_shards) and its own properties; the rebased
serialiser (blkjson.h blk_len / blk_emit with BlkBases: what
k_blk_body_hash_rb runs per lane) on the host, given only copies of a shard's
slices and its bases (tests/emu_blkshards), against hashlib over the oracle's
bodies; and both through an ASan + UBSan stand-alone driver
(tests/emu_blkshards/fuzz_main.cpp, run as a subprocess)."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from babble_amd import native, shard
from babble_amd.batch import BlockBatchBuilder
from babble_amd.verifier import plan_block_shards
from tests import block_cases as BC
from tests.emu_blkshards import emu_blkshards

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_blkshards")
EXE = os.path.join(HERE, "_build", "blkshardfuzz")


def _c_plan(item_block, n_blocks, D, null_items=False):
    ib = np.ascontiguousarray(item_block, np.uint32)
    b = native.BvBlockBatch()
    b.n_blocks, b.n_items = n_blocks, len(ib)
    # (an empty batch still passes a valid pointer)
    b.item_block = None if null_items else (ib.ctypes.data if ib.size else np.zeros(1, np.uint32).ctypes.data)
    bb = np.zeros(D + 1, np.uint64)
    bi = np.zeros(D + 1, np.uint64)
    rc = native.lib().bv_plan_block_shards(ctypes.byref(b), D, bb.ctypes.data, bi.ctypes.data)
    return rc, bb.tolist(), bi.tolist()


def _cases():
    """1,000 random (D, n_blocks, item_block): 0..60 blocks, D in [1, 9], 0..5
    items per block with item-less runs at either end and between; every
    fifth case has no items, every seventh puts all items on one block, every
    fourth is shuffled (unsorted when it names two blocks)."""
    rng = np.random.default_rng(77)
    out = []
    for t in range(1000):
        n = int(rng.integers(0, 61))
        D = int(rng.integers(1, 10))
        per = rng.integers(0, 6, size=n) * (rng.random(n) < 0.7)
        if n:
            a, z = sorted(int(x) for x in rng.integers(0, n + 1, size=2))
            if t % 3 == 0:
                per[:a] = 0
                per[z:] = 0
        if t % 5 == 0:
            per[:] = 0
        ib = np.repeat(np.arange(n, dtype=np.uint32), per.astype(np.int64))
        if t % 7 == 0 and n:
            ib = np.full(int(rng.integers(0, 40)), int(rng.integers(0, n)), np.uint32)
        if t % 4 == 1:
            ib = rng.permutation(ib)
        out.append((D, n, ib))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _check_properties(rc, bb, bi, D, n, ib):
    ni = len(ib)
    unsorted = bool(ni > 1 and np.any(ib[1:] < ib[:-1]))
    assert rc == int(unsorted)
    if unsorted:
        assert bb == [0] + [n] * D and bi == [0] + [ni] * D
        return
    assert bb[0] == 0 and bb[-1] == n and all(a <= b for a, b in zip(bb, bb[1:]))  # a partition of the blocks
    assert bi[0] == 0 and bi[-1] == ni and all(a <= b for a, b in zip(bi, bi[1:]))
    assert bi == shard.plan_shards(ib, D)  # bv_plan_shards' item bounds
    for d in range(D):
        s = ib[bi[d]:bi[d + 1]]
        assert np.all((s >= bb[d]) & (s < bb[d + 1]))  # a block's items are never split from it
        if d and 0 < bi[d] < ni:
            assert ib[bi[d]] != ib[bi[d] - 1]


def test_plan_c_equals_model_and_properties(cases):
    n_unsorted = n_empty = n_more_shards = n_one_block = 0
    for D, n, ib in cases:
        rc, bb, bi = _c_plan(ib, n, D)
        uns, mbb, mbi = shard.plan_block_shards(ib, n, D)
        assert (rc, bb, bi) == (int(uns), mbb, mbi), (D, n, ib.tolist())
        _check_properties(rc, bb, bi, D, n, ib)
        n_unsorted += rc
        n_empty += len(ib) == 0
        n_more_shards += D > n
        n_one_block += len(ib) > 1 and len(set(ib.tolist())) == 1
    assert n_unsorted > 100 and n_empty > 150 and n_more_shards > 20 and n_one_block > 50


def test_plan_fixed_cases():
    # 4 blocks x 3 items over 3 shards: cut at the first block change at or after n g / 3
    ib = np.repeat(np.arange(4, dtype=np.uint32), 3)
    assert _c_plan(ib, 4, 3) == (0, [0, 2, 3, 4], [0, 6, 9, 12])
    # item-less blocks before the first and after the last item, and between shards (to the earlier shard)
    ib = np.array([2, 2, 2, 5, 5, 5], np.uint32)
    assert _c_plan(ib, 9, 2) == (0, [0, 5, 9], [0, 3, 6])
    # no items: every block on shard 0 ... the partition still covers [0, n)
    rc, bb, bi = _c_plan(np.zeros(0, np.uint32), 7, 3)
    assert rc == 0 and bb[0] == 0 and bb[-1] == 7 and bi == [0, 0, 0, 0]
    # more shards than blocks; one block holding all items
    rc, bb, bi = _c_plan(np.zeros(10, np.uint32), 1, 4)
    assert rc == 0 and bi == [0, 10, 10, 10, 10] and bb[0] == 0 and bb[-1] == 1
    assert _c_plan(np.zeros(0, np.uint32), 0, 2) == (0, [0, 0, 0], [0, 0, 0])
    # unsorted: whole-batch bounds, returns 1
    assert _c_plan(np.array([1, 0, 1], np.uint32), 3, 3) == (1, [0, 3, 3, 3], [0, 3, 3, 3])


def test_plan_bad_arguments():
    L = native.lib()
    ib = np.array([0, 1, 2], np.uint32)
    assert _c_plan(ib, 3, 2)[0] == 0
    assert _c_plan(ib, 2, 2)[0] == native.BV_E_ARGS  # item_block >= n_blocks
    assert _c_plan(ib, 3, 2, null_items=True)[0] == native.BV_E_ARGS
    assert _c_plan(ib, 3, 0)[0] == native.BV_E_ARGS
    b = native.BvBlockBatch()
    x = np.zeros(4, np.uint64)
    p = x.ctypes.data
    assert L.bv_plan_block_shards(None, 2, p, p) == native.BV_E_ARGS
    assert L.bv_plan_block_shards(ctypes.byref(b), 2, None, p) == native.BV_E_ARGS
    assert L.bv_plan_block_shards(ctypes.byref(b), 2, p, None) == native.BV_E_ARGS
    assert L.bv_plan_block_shards(ctypes.byref(b), -3, p, p) == native.BV_E_ARGS


def test_plan_python_binding_reads_only_counts_and_items():
    case = BC.signed_case(BC.random_bodies(30, seed=3), lambda b: b % 4, 5)
    uns, bb, bi = plan_block_shards(case.fields, 3)
    assert (uns, bb.tolist(), bi.tolist()) == shard.plan_block_shards(case.fields.item_block, 30, 3) and not uns
    sh = BC.signed_case(BC.random_bodies(30, seed=3), 2, 5, shuffle=True)
    uns, bb, bi = plan_block_shards(sh.fields, 2)
    assert uns and bb.tolist() == [0, 30, 30] and bi.tolist() == [0, 60, 60]


# ---------------------------------------------------------------------------
# The rebased serialiser, given only copies of a shard's slices and its bases
# ---------------------------------------------------------------------------
def _pack(bodies):
    kb = BlockBatchBuilder()
    for b in bodies:
        kb.add_block(b)
    return kb.pack()


def _check_split(pb, want, bounds):
    for d in range(len(bounds) - 1):
        b0, b1 = bounds[d], bounds[d + 1]
        sl, bases = emu_blkshards.slice_blocks(pb, b0, b1, 0, 0)
        assert sl.n_blocks == b1 - b0
        dig, lens = emu_blkshards.body_hash(sl, bases, b0, b1)
        for b in range(b0, b1):
            assert dig[b - b0].tobytes() == want[b][0] and int(lens[b - b0]) == want[b][1], (bounds, b)


def _forty(bodies):
    pb = _pack(bodies)
    want = [(hashlib.sha256(r).digest(), len(r)) for r in (b.Marshal() for b in bodies)]
    return pb, want


def test_rebased_serialiser_every_cut_of_a_three_way_split():
    """40-block batches of grid and random bodies; both cut points of a 3-way
    split moved over every position (empty shards included): each shard's
    digests and lengths, from copies of its slices and its bases only, equal
    hashlib over the oracle's bodies."""
    grid = BC.grid_bodies()
    batches = [grid[i:i + 40] for i in (0, 300, 856)] + [BC.random_bodies(40, seed=s) for s in (11, 12)]
    for bodies in batches:
        pb, want = _forty(bodies)
        assert len(bodies) == 40
        for c1 in range(41):
            for c2 in range(c1, 41):
                _check_split(pb, want, [0, c1, c2, 40])


def test_rebased_serialiser_whole_grid_in_shards():
    """Every grid body and 300 random ones through a 3-shard cut: all bases
    non-zero in the later shards, nil lists and fragments on both sides."""
    for bodies in (BC.grid_bodies(), BC.random_bodies(300, seed=21)):
        pb, want = _forty(bodies)
        n = len(bodies)
        bounds = [0, n // 3 + 1, 2 * n // 3 + 2, n]
        _check_split(pb, want, bounds)
        sl, bases = emu_blkshards.slice_blocks(pb, bounds[1], bounds[2], 0, 0)
        assert bases[0] > 0 and bases[1] > 0 and bases[2] > 0 and bases[3] > 0
        if pb.itx_off is not None:
            assert int(pb.itx_off[-1]) > 0 and int(pb.rcpt_off[-1]) > 0


def test_sanitized_plan_and_rebased_serialiser():
    """The stand-alone ASan + UBSan driver: the plan over exactly-sized arrays
    and every shard's bodies from exactly-sized copies of its slices."""
    subprocess.run(["make", "-s", "-C", HERE, "fuzz"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        p = subprocess.run([EXE, str(seed), "150"], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
        f = p.stdout.split()
        assert f[0] == "ok" and int(f[1]) == 150 and int(f[2]) > 150 and int(f[3]) > 1000, p.stdout


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def test_new_symbols_resolve_and_reject_null():
    L = native.lib()
    for name in ("bv_group_verify_blocks", "bv_plan_block_shards"):
        assert name in native.EXPORTS and getattr(L, name) is not None
    assert L.bv_group_verify_blocks(None, None, None, None) == native.BV_E_ARGS
    b = native.BvBlockBatch()
    r = native.BvResult()
    assert L.bv_group_verify_blocks(None, ctypes.byref(b), ctypes.byref(r), None) == native.BV_E_ARGS
    import babble_amd

    assert babble_amd.Group.verify_blocks and babble_amd.Group.verify_blocks_into
    assert babble_amd.plan_block_shards is plan_block_shards
