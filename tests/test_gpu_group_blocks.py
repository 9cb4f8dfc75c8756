"""bv_group_verify_blocks on the GPU: blocks from their fields, sharded by
block across the group's device slots.  Every group here is made of logical
shards of device 0 (one ctx each): the shard plan, the concurrent per-shard
staging threads, the rebased kernels (k_blk_body_hash_rb, k_blk_item_rebase,
k_sig_decode_rb), the per-shard tally and the shifted bit merge are the
multi-device code path, only the gather is device copies instead of one RCCL
all-gather.  BlockCase.oracle() (the C oracle over the Go-semantics oracle's
bodies), its digests and valid_count() are the judge; Verifier.verify_blocks
on one context is a second witness."""
import dataclasses
import hashlib
import random

import numpy as np
import pytest

from babble_amd import hashgraph as H
from babble_amd import native, shard
from babble_amd.verifier import BlockVerifyResult, Group, PinnedArena, Verifier
from oracle import gosemantics as G
from tests import block_cases as BC
from tests.test_gpu_block_fields import cached, check, grid_case
from tests.test_hostfuzz import _sig_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def v0():
    v = Verifier(0)
    yield v
    v.close()


@pytest.fixture()
def g3(monkeypatch):
    """Three logical shards of device 0 whose contexts never take the
    one-launch small path (BV_SMALL is read at bv_create): every batch sorted
    by block is sharded, however small."""
    monkeypatch.setenv("BV_SMALL", "0")
    g = Group([0, 0, 0])
    yield g
    g.close()


def plan(c, D):
    uns, bb, bi = shard.plan_block_shards(c.fields.item_block, c.fields.n_blocks, D)
    assert not uns
    return bb, bi


def same(a, b, what=""):
    assert np.array_equal(a.msg_hash, b.msg_hash), what
    assert np.array_equal(a.status, b.status) and np.array_equal(a.accept_bits, b.accept_bits), what
    assert np.array_equal(a.valid_count, b.valid_count), what


def test_grid_across_three_shards(g3, v0):
    c = cached("grid", grid_case)
    bb, bi = plan(c, 3)
    assert bi == [0, 897, 1794, 2688] and all(x % 64 for x in bi[1:3])  # the shifted merge
    assert bb == [0, 299, 598, 897]
    res = g3.verify_blocks(c.fields)
    check(c, res, "grid")
    assert set(np.unique(res.status).tolist()) == {0, 1} and res.valid_count[896] == 0
    for d in range(3):
        assert g3.timing(d)["ms_h2d"] > 0  # every slot ran the bulk pipeline
    same(res, v0.verify_blocks(c.fields), "single context")


@pytest.mark.parametrize("n_blocks", [1, 63, 64, 65, 130, 300])
def test_block_counts_across_lane_and_workgroup_boundaries(g3, v0, n_blocks):
    """One lane per block in workgroups of 64 lanes, per shard: shards of 0, 1
    and a few blocks, and shards on both sides of a wave; 1-5 items per block."""
    def make():
        rng = random.Random(n_blocks)
        return BC.signed_case(BC.random_bodies(n_blocks, seed=140 + n_blocks), lambda b: rng.randint(1, 5), 8,
                              seed=n_blocks, corrupt=0.2)

    c = cached(("group lanes", n_blocks), make)
    bb, bi = plan(c, 3)
    if n_blocks == 1:
        assert bb == [0, 0, 1, 1]  # two empty shards, the first among them
    res = g3.verify_blocks(c.fields)
    check(c, res, f"{n_blocks} blocks, block bounds {bb}")
    same(res, v0.verify_blocks(c.fields), "single context")


def test_item_less_blocks_at_the_ends_and_at_the_cuts(g3):
    sig = set(range(5, 25)) | set(range(30, 50)) | set(range(55, 75))
    c = cached("group itemless", lambda: BC.signed_case(BC.random_bodies(80, seed=150),
                                                        lambda b: 3 if b in sig else 0, 8, seed=151, corrupt=0.2))
    bb, bi = plan(c, 3)
    assert bb == [0, 30, 55, 80] and bi == [0, 60, 120, 180]  # blocks 25-29 and 50-54: to the earlier shard
    res = g3.verify_blocks(c.fields)
    check(c, res, "item-less blocks")
    assert not res.valid_count[[b for b in range(80) if b not in sig]].any() and res.valid_count.any()
    # no item at all: every block is hashed (on slot 0: the partition gives it all of them)
    c0 = cached("group no items", lambda: BC.BlockCase(c.bodies, [], 8))
    r0 = g3.verify_blocks(c0.fields)
    assert np.array_equal(r0.msg_hash, c.digests) and r0.status.size == 0 and not r0.valid_count.any()


def test_long_bodies_in_the_second_and_third_shard(g3, v0):
    """Bodies of 16,384 bytes (the longest a lane hashes) and 16,385 bytes (the
    shortest the host hashes) under a non-zero block base: the long-block list
    and the host hash path of shards 1 and 2 (and of shard 0, base zero)."""
    def make():
        bodies = BC.random_bodies(30, seed=160)
        for b, n in ((3, 16385), (12, 16384), (14, 16385), (19, 16385), (20, 16385), (22, 16384), (29, 16385)):
            bodies[b] = BC.body_of_length(n)
        return BC.signed_case(bodies, 3, 8, seed=161, corrupt=0.2)

    c = cached("group long", make)
    bb, bi = plan(c, 3)
    assert bb == [0, 10, 20, 30] and bi == [0, 30, 60, 90]
    assert [len(c.raw[b]) for b in (12, 14, 19, 20, 22, 29)] == [16384, 16385, 16385, 16385, 16384, 16385]
    res = g3.verify_blocks(c.fields)
    check(c, res, "long bodies")
    same(res, v0.verify_blocks(c.fields), "single context")


def _adversarial_sorted():
    """The corruption classes of block signatures, items sorted by block: bad
    text, the range classes of r and s, malformed keys, bodies changed after
    signing."""
    rng = random.Random(170)
    nv = 8
    vs = BC.validators(nv)
    bodies = BC.synth_like_bodies(60, n_tx=3, tx_bytes=40, seed=171)
    digests = [hashlib.sha256(b.Marshal()).digest() for b in bodies]
    extra = [b"", b"\x04" + bytes(64), vs[0][1][:33], vs[1][1][:64] + bytes([vs[1][1][64] ^ 1]), b"\x03" + vs[2][1][1:]]
    corpus = _sig_cases(random.Random(7))
    N = G.N
    ranges = [G.EncodeSignature(0, 5), G.EncodeSignature(5, 0), G.EncodeSignature(N, 5), G.EncodeSignature(5, N),
              G.EncodeSignature(N + 1, N - 1), "-5|7", "7|-5", G.EncodeSignature(2**256, 1), "|5", "5|", "zz|!"]
    items = []
    for b in range(60):
        for v in sorted(rng.sample(range(nv), 6)):
            text = BC.sign(vs[v][0], digests[b], rng.randrange(4)).encode()
            key = v
            c = rng.random()
            if c < 0.12:
                text = bytes(rng.choice(corpus))
            elif c < 0.24:
                text = rng.choice(ranges).encode()
            elif c < 0.36:
                key = nv + rng.randrange(len(extra))
            elif c < 0.42:
                text = text[:-1] + (b"1" if text[-1:] != b"1" else b"2")
            items.append((b, key, text))
    mutated = list(bodies)
    for b in (3, 21, 41, 59):  # signed, then one field changed: every signature of the block is rejected
        m = bodies[b]
        mutated[b] = G.BlockBody(m.Index, m.RoundReceived, m.Timestamp + 1, m.StateHash, m.FrameHash, m.PeersHash,
                                 m.Transactions, m.InternalTransactions, m.InternalTransactionReceipts)
    return BC.BlockCase(mutated, items, nv, extra)


@pytest.mark.parametrize("form", ["text", "decoded"])
def test_signature_forms_every_status(g3, form):
    """Signature text decoded per shard (k_sig_decode_rb through the whole
    batch's offsets), and host-decoded r_be / s_be / pre sliced per shard."""
    c = cached("group adversarial", _adversarial_sorted)
    _, st, _ = c.oracle()
    assert set(np.unique(st).tolist()) == {0, 1, 2, 3}, np.bincount(st, minlength=4)
    bb, bi = plan(c, 3)
    assert all(0 < x < c.n_items for x in bi[1:3]) and int(c.fields.sig_off[bi[1]]) > 0
    pb = c.fields if form == "text" else c.fields.decoded()
    assert (pb.sig_text is None) == (form == "decoded")
    check(c, g3.verify_blocks(pb), form)


def test_unsharded_routes_stay_on_slot_0(v0):
    """Items not sorted by block, and a batch the single context runs on its
    one-launch small path: one bv_verify_blocks call on slot 0, the single
    context's results."""
    sh = cached("group shuffled", lambda: BC.signed_case(BC.random_bodies(200, seed=180), 3, 8, seed=181,
                                                         shuffle=True, corrupt=0.2))
    assert (np.diff(sh.fields.item_block.astype(np.int64)) < 0).any()
    small = cached("group small", lambda: BC.signed_case(BC.random_bodies(2, seed=182), 50, 100, seed=183,
                                                         corrupt=0.2))
    g = Group([0, 0, 0])
    try:
        res = g.verify_blocks(sh.fields)
        check(sh, res, "shuffled items")
        assert g.timing(0)["ms_h2d"] > 0 and g.timing(1)["ms_host"] == 0 and g.timing(2)["ms_host"] == 0
        same(res, v0.verify_blocks(sh.fields), "single context")
        res = g.verify_blocks(small.fields)
        check(small, res, "small batch")
        one = v0.verify_blocks(small.fields)
        t = v0.timing()
        same(res, one, "single context, small")
        assert t["ms_h2d"] == 0 and g.timing(0)["ms_h2d"] == 0  # both took the one-launch path
        assert g.timing(1)["ms_host"] == 0 and g.timing(2)["ms_host"] == 0
    finally:
        g.close()


def test_pinned_in_place_and_output_forms(g3):
    c = cached("grid", grid_case)
    n, ni = c.fields.n_blocks, c.n_items
    arena = PinnedArena()
    try:
        for pb in (arena.block_batch(c.fields), arena.block_batch(c.fields.decoded())):
            res = BlockVerifyResult(arena.array((n, 32), np.uint8), arena.array(ni, np.uint8),
                                    arena.array((ni + 63) // 64, np.uint64), arena.array(n, np.uint32))
            res.status[:] = 0xEE
            res.valid_count[:] = 0xEEEEEEEE
            g3.verify_blocks_into(pb, res)
            check(c, res, "pinned")
        full = res
        # status == NULL with valid_count: no per-item array comes back
        r1 = BlockVerifyResult(arena.array((n, 32), np.uint8), None, arena.array((ni + 63) // 64, np.uint64),
                               arena.array(n, np.uint32))
        g3.verify_blocks_into(pb, r1)
        assert np.array_equal(r1.valid_count, c.valid_count()) and np.array_equal(r1.msg_hash, c.digests)
        assert np.array_equal(r1.accept_bits, full.accept_bits)
        # valid_count == NULL; and digests / bits NULL too
        r2 = BlockVerifyResult(arena.array((n, 32), np.uint8), arena.array(ni, np.uint8),
                               arena.array((ni + 63) // 64, np.uint64), None)
        g3.verify_blocks_into(pb, r2)
        assert np.array_equal(r2.status, full.status) and np.array_equal(r2.msg_hash, c.digests)
        assert np.array_equal(r2.accept_bits, full.accept_bits)
        r3 = BlockVerifyResult(None, None, None, arena.array(n, np.uint32))
        g3.verify_blocks_into(pb, r3)
        assert np.array_equal(r3.valid_count, c.valid_count())
        # the pageable forms of Group.verify_blocks
        a = g3.verify_blocks(c.fields, status=False)
        b = g3.verify_blocks(c.fields, counts=False)
        assert a.status is None and np.array_equal(a.valid_count, c.valid_count()) and b.valid_count is None
        assert np.array_equal(b.status, full.status) and np.array_equal(a.accept_bits, full.accept_bits)
    finally:
        arena.close()


def test_key_cache_registered_validators():
    c = cached("group kc", lambda: BC.signed_case(BC.synth_like_bodies(500, n_tx=4, tx_bytes=64, seed=80), 4, 4,
                                                  seed=81, corrupt=0.05))
    assert c.n_items == 2000
    g = Group([0, 0], flags=native.F_KEY_CACHE)
    try:
        g.register_keys([pub for _, pub in BC.validators(4)])
        res = g.verify_blocks(c.fields)
        for slot in (0, 1):
            t = g.timing(slot)
            assert t["key_path"] == 22 and t["kc_hits"] == 4, (slot, t)
        check(c, res, "key cache")
    finally:
        g.close()


def test_validation_error_then_a_valid_call(g3):
    c = cached("grid", grid_case)
    pb = c.fields
    bad = pb.item_block.copy()
    bad[1500] = pb.n_blocks  # item_block >= n_blocks
    with pytest.raises(native.BvError) as e:
        g3.verify_blocks(dataclasses.replace(pb, item_block=bad))
    assert e.value.code == native.BV_E_ARGS and "item index out of range" in str(e.value)
    off = pb.hash_off.copy()
    off[700], off[701] = off[701] + 1, off[700]
    with pytest.raises(native.BvError) as e:
        g3.verify_blocks(dataclasses.replace(pb, hash_off=off))
    assert e.value.code == native.BV_E_ARGS and "hash_off not monotone" in str(e.value)
    check(c, g3.verify_blocks(pb), "after the refused batches")


def test_check_blocks_through_the_group(g3, v0):
    """hashgraph.check_blocks with group=: the same verdicts as without, on
    blocks that pass, blocks under the trust count, and a wrong peer set."""
    nv = 4
    vs = BC.validators(nv)
    ps = H.PeerSet([H.Peer(PubKeyHex=H.EncodeToString(pub)) for _, pub in vs])  # TrustCount 2
    ph = ps.Hash(v0)
    rng = random.Random(190)
    blocks, kinds = [], []
    for i in range(120):
        kind = ("ok", "short", "wrong")[0 if i % 5 < 3 else 1 if i % 5 == 3 else 2]
        body = H.BlockBody(Index=i, RoundReceived=i + 1, Timestamp=1_600_000_000 + i, StateHash=b"s" * 32,
                           FrameHash=None, PeersHash=ph if kind != "wrong" else b"\x00" * 32,
                           Transactions=[b"tx%d" % i, None, b""], InternalTransactions=None,
                           InternalTransactionReceipts=[])
        blk = H.Block(Body=body)
        dig = hashlib.sha256(body.Marshal()).digest()
        spoil = set(rng.sample(range(nv), 2)) if kind == "short" else set()
        for v, (d, pub) in enumerate(vs):
            text = BC.sign(d, dig, rng.randrange(4))
            if v in spoil:
                text = text[:-1] + ("1" if text[-1] != "1" else "2")
            blk.Signatures[H.EncodeToString(pub)] = text
        blocks.append(blk)
        kinds.append(kind)
    sets = [ps] * len(blocks)
    want = H.check_blocks(blocks, sets, v0)
    got = H.check_blocks(blocks, sets, v0, group=g3)
    assert got == want
    for kind, w in zip(kinds, want):
        assert w == {"ok": None, "short": "Not enough valid signatures: got 2, need 2", "wrong": "Wrong PeerSet"}[kind]
    for d in range(3):
        assert g3.timing(d)["ms_h2d"] > 0  # the one call was sharded
