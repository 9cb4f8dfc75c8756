"""bv_verify_blocks on the device: BlockBody JSON built and hashed from the
blocks' fields (k_blk_body_hash), the block signatures verified as items, and
CheckBlock's tally per block (k_blk_tally).

Judge: oracle.coracle.verify_batch over the ORACLE's serialised bodies
(oracle/gosemantics.py BlockBody.Marshal) with the signature texts decoded on
the host; digests, statuses and accept bits must be bit-exact and valid_count
must equal numpy.bincount of the ACCEPT items by block.  The 30,000-item bulk
batch is judged item for item by bv_verify_batch_text over the oracle's bodies
(the entry this one is modelled on), its digests by hashlib, and by the oracle
on a fixed sample of 2,000 items (the oracle verifies ~4,000 items a second).
Workloads: tests/block_cases.py."""
import hashlib
import random

import numpy as np
import pytest

from babble_amd import native
from babble_amd.verifier import BlockVerifyResult, PinnedArena, Verifier
from oracle import gosemantics as G
from tests import block_cases as BC
from tests.test_hostfuzz import _sig_cases

pytestmark = pytest.mark.gpu

_cases = {}


def cached(name, make):
    if name not in _cases:
        _cases[name] = make()
    return _cases[name]


@pytest.fixture(scope="module")
def v0():
    v = Verifier(0)
    yield v
    v.close()


def check(c: BC.BlockCase, res, what="", counts=True):
    h, st, bits = c.oracle()
    assert np.array_equal(h, c.digests), what  # the oracle's digests are hashlib's
    assert np.array_equal(res.msg_hash, h), (what, np.flatnonzero((res.msg_hash != h).any(axis=1))[:8])
    assert np.array_equal(res.status, st), (what, np.flatnonzero(res.status != st)[:8])
    assert np.array_equal(res.accept_bits, bits), what
    if counts:
        assert res.valid_count.dtype == np.uint32 and np.array_equal(res.valid_count, c.valid_count()), what


def grid_case():
    bodies = BC.grid_bodies() + [G.BlockBody(5, 6, 7, b"no", b"item", None, [b"here"], None, None)]
    return BC.signed_case(bodies, lambda b: 0 if b == len(bodies) - 1 else 3, 8, seed=11, corrupt=0.1)


def test_grid_batch_three_items_per_block(v0):
    c = cached("grid", grid_case)
    assert c.fields.n_blocks == 897 and c.n_items == 3 * 896
    assert not (c.fields.item_block == 896).any()  # the last block has no item: still hashed, count 0
    res = v0.verify_blocks(c.fields)
    t = v0.timing()
    check(c, res, "grid")
    assert t["ms_h2d"] > 0, t  # the bulk pipeline: the bodies were built on the device
    assert res.valid_count[896] == 0 and set(np.unique(res.status).tolist()) == {0, 1}


@pytest.mark.parametrize("n_blocks", [1, 63, 64, 65, 257])
def test_lane_and_workgroup_boundaries(v0, n_blocks):
    """One lane per block in workgroups of 64 (or 256) lanes: block counts on
    both sides of a wave and past four waves; 1-5 items per block, in
    shuffled block order (the tally's runs are then mostly one lane long)."""
    def make():
        rng = random.Random(n_blocks)
        return BC.signed_case(BC.random_bodies(n_blocks, seed=40 + n_blocks), lambda b: rng.randint(1, 5), 8,
                              seed=n_blocks, shuffle=True, corrupt=0.2)

    c = cached(("lanes", n_blocks), make)
    assert n_blocks == 1 or (np.diff(c.fields.item_block.astype(np.int64)) < 0).any()
    check(c, v0.verify_blocks(c.fields), f"{n_blocks} blocks")


def test_long_bodies_host_path_equals_device_path(v0):
    """Bodies of exactly 16,384 bytes (the longest a lane hashes), 16,385
    bytes (the shortest the host hashes) and ~40 KB, short ones between."""
    def make():
        short = BC.random_bodies(6, seed=50)
        bodies = [short[0], BC.body_of_length(16384), short[1], BC.body_of_length(16385), short[2], short[3],
                  BC.body_of_length(40001), short[4], BC.body_of_length(16385), short[5]]
        return BC.signed_case(bodies, 3, 8, seed=51, corrupt=0.2)

    c = cached("long", make)
    assert [len(c.raw[i]) for i in (1, 3, 6, 8)] == [16384, 16385, 40001, 16385]
    assert max(len(c.raw[i]) for i in (0, 2, 4, 5, 7, 9)) < 4096
    res = v0.verify_blocks(c.fields)
    t = v0.timing()
    check(c, res, "long bodies")
    assert t["ms_h2d"] > 0, t
    # in shuffled item order and without items
    c2 = cached("long_shuffled", lambda: BC.signed_case(c.bodies, 3, 8, seed=52, shuffle=True))
    check(c2, v0.verify_blocks(c2.fields), "long bodies, shuffled items")
    c3 = cached("long_no_items", lambda: BC.BlockCase(c.bodies, [], 8))
    r3 = v0.verify_blocks(c3.fields)
    assert np.array_equal(r3.msg_hash, c.digests) and r3.status.size == 0 and not r3.valid_count.any()


@pytest.mark.parametrize("n_items", [1, 4, 100, 256])
def test_small_batches_take_the_text_entrys_route(v0, n_items):
    """Where bv_verify_batch_text takes the one-launch path so does
    bv_verify_blocks, over bodies it serialises on the host: the same
    statuses as verify_text over the host-serialised bodies, and ms_h2d == 0
    (nothing staged) for both."""
    def make():
        n_blocks, per = {1: (1, 1), 4: (1, 4), 100: (2, 50), 256: (4, 64)}[n_items]
        return BC.signed_case(BC.random_bodies(n_blocks, seed=60 + n_items), per, 100 if per > 8 else 8,
                              seed=61 + n_items, corrupt=0.2)

    c = cached(("small", n_items), make)
    assert c.n_items == n_items
    host_bodies = c.fields.bodies()  # bv_block_bodies
    assert host_bodies[0].tobytes() == b"".join(c.raw)
    ref = v0.verify_text(c.fields.text_batch(host_bodies))
    t_ref = v0.timing()
    res = v0.verify_blocks(c.fields)
    t = v0.timing()
    check(c, res, f"{n_items} items")
    assert np.array_equal(res.status, ref.status) and np.array_equal(res.msg_hash, ref.msg_hash)
    assert np.array_equal(res.accept_bits, ref.accept_bits)
    assert t_ref["ms_h2d"] == 0 and t["ms_h2d"] == 0, (t_ref, t)


def adversarial_case():
    """The C4 corruption classes on block signatures: bad text, the range
    classes of r and s, malformed keys, a body field mutated after signing."""
    rng = random.Random(70)
    nv = 8
    vs = BC.validators(nv)
    bodies = BC.synth_like_bodies(60, n_tx=3, tx_bytes=40, seed=71)
    digests = [hashlib.sha256(b.Marshal()).digest() for b in bodies]
    extra = [b"", b"\x04" + bytes(64), vs[0][1][:33], vs[1][1][:64] + bytes([vs[1][1][64] ^ 1]), b"\x03" + vs[2][1][1:]]
    corpus = _sig_cases(random.Random(7))
    N = G.N
    ranges = [G.EncodeSignature(0, 5), G.EncodeSignature(5, 0), G.EncodeSignature(N, 5), G.EncodeSignature(5, N),
              G.EncodeSignature(N + 1, N - 1), "-5|7", "7|-5", G.EncodeSignature(2**256, 1), "|5", "5|", "zz|!"]
    items = []
    for b in range(60):
        for v in rng.sample(range(nv), 6):
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
    for b in (3, 17, 31, 59):  # signed, then one field changed: every signature of the block is rejected
        m = bodies[b]
        mutated[b] = G.BlockBody(m.Index, m.RoundReceived, m.Timestamp + 1, m.StateHash, m.FrameHash, m.PeersHash,
                                 m.Transactions, m.InternalTransactions, m.InternalTransactionReceipts)
    rng.shuffle(items)
    return BC.BlockCase(mutated, items, nv, extra)


@pytest.mark.parametrize("form", ["text", "decoded"])
def test_adversarial_items_every_status(v0, form):
    c = cached("adversarial", adversarial_case)
    _, st, _ = c.oracle()
    assert set(np.unique(st).tolist()) == {0, 1, 2, 3}, np.bincount(st, minlength=4)
    for b in (3, 17, 31, 59):
        assert not (st[c.fields.item_block == b] == 1).any()
    pb = c.fields if form == "text" else c.fields.decoded()
    assert (pb.sig_text is None) == (form == "decoded")
    res = v0.verify_blocks(pb)
    t = v0.timing()
    check(c, res, form)
    assert t["ms_h2d"] > 0, t


def test_key_cache_registered_validators():
    def make():
        return BC.signed_case(BC.synth_like_bodies(500, n_tx=4, tx_bytes=64, seed=80), 4, 4, seed=81, corrupt=0.05)

    c = cached("kc", make)
    assert c.n_items == 2000
    v = Verifier(0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys([pub for _, pub in BC.validators(4)])
        res = v.verify_blocks(c.fields)
        t = v.timing()
        check(c, res, "key cache")
        assert t["key_path"] == 22 and t["kc_hits"] == 4 and t["kc_builds"] == 0, t
    finally:
        v.close()


def test_output_forms_write_the_same_values(v0):
    c = cached("grid", grid_case)
    full = v0.verify_blocks(c.fields)
    check(c, full, "all outputs")
    # status == NULL with valid_count: no per-item array comes back
    r1 = v0.verify_blocks(c.fields, counts=True, status=False)
    assert r1.status is None and np.array_equal(r1.valid_count, full.valid_count)
    assert np.array_equal(r1.msg_hash, full.msg_hash) and np.array_equal(r1.accept_bits, full.accept_bits)
    # valid_count == NULL
    r2 = v0.verify_blocks(c.fields, counts=False)
    assert r2.valid_count is None and np.array_equal(r2.status, full.status)
    assert np.array_equal(r2.msg_hash, full.msg_hash) and np.array_equal(r2.accept_bits, full.accept_bits)
    # every result buffer, then every input too, in pinned memory
    arena = PinnedArena()
    try:
        n, ni = c.fields.n_blocks, c.n_items
        for pb in (c.fields, arena.block_batch(c.fields), arena.block_batch(c.fields.decoded())):
            res = BlockVerifyResult(arena.array((n, 32), np.uint8), arena.array(ni, np.uint8),
                                    arena.array((ni + 63) // 64, np.uint64), arena.array(n, np.uint32))
            res.status[:] = 0xEE
            res.valid_count[:] = 0xEEEEEEEE
            v0.verify_blocks_into(pb, res)
            check(c, res, "pinned")
        # the small path's forms: same values as well
        s = cached("small_outputs", lambda: BC.signed_case(BC.random_bodies(2, seed=160), 50, 100, seed=161,
                                                           corrupt=0.2))
        a = v0.verify_blocks(s.fields)
        b = v0.verify_blocks(s.fields, status=False)
        d = v0.verify_blocks(s.fields, counts=False)
        check(s, a, "small")
        assert b.status is None and np.array_equal(b.valid_count, a.valid_count) and d.valid_count is None
        assert np.array_equal(d.status, a.status) and np.array_equal(b.accept_bits, a.accept_bits)
    finally:
        arena.close()


def test_pinned_and_pageable_arrays_past_the_one_copy_limit(monkeypatch):
    """64 blocks x 4 validators with 1.2 MB of tx_bytes (a layout past the 1 MiB
    one-copy limit; 40 bodies are long enough for the host to hash), tx_bytes in
    bv_host_alloc memory and every other array pageable: in the block-field
    phase one array crosses by DMA from where it lies and its neighbours
    through the staging block one by one.  Equal to the oracle and to the
    all-pageable call; a tenth of the signatures is corrupted."""
    import dataclasses

    c = cached("mixed", lambda: BC.signed_case(BC.synth_like_bodies(40, n_tx=16, tx_bytes=1500, seed=3) +
                                               BC.synth_like_bodies(24, n_tx=9, tx_bytes=1200, seed=4), 4, 4, seed=77,
                                               corrupt=0.1))
    assert c.fields.tx_bytes.nbytes > 1_200_000 and c.n_items == 256
    assert 0 < int((c.oracle()[1] != 1).sum()) < 64
    monkeypatch.setenv("BV_SMALL", "0")  # (256 items: the bulk pipeline whatever the routing rule says)
    v = Verifier(0)
    arena = PinnedArena()
    try:
        mixed = dataclasses.replace(c.fields, tx_bytes=arena.copy(c.fields.tx_bytes))
        res = v.verify_blocks(mixed)
        assert v.timing()["ms_h2d"] > 0
        check(c, res, "tx_bytes pinned")
        ref = v.verify_blocks(c.fields)
        check(c, ref, "pageable")
        assert np.array_equal(res.status, ref.status) and np.array_equal(res.msg_hash, ref.msg_hash)
    finally:
        v.close()
        arena.close()


def test_validation_errors_then_a_valid_call(v0):
    import ctypes

    c = cached("grid", grid_case)
    pb = c.fields
    n, ni = pb.n_blocks, pb.n_items

    def call(edit):
        keep = []
        cb = pb.c_struct(keep)
        edit(cb, keep)
        h = np.zeros((n, 32), np.uint8)
        st = np.zeros(ni, np.uint8)
        bits = np.zeros((ni + 63) // 64, np.uint64)
        vc = np.zeros(n, np.uint32)
        r = native.BvResult(h.ctypes.data, st.ctypes.data, bits.ctypes.data)
        rc = v0._L.bv_verify_blocks(v0._ctx, ctypes.byref(cb), ctypes.byref(r), vc.ctypes.data)
        return rc, v0._L.bv_last_error(v0._ctx).decode(errors="replace")

    def swap(name, fn):
        def edit(cb, keep):
            a = np.array(getattr(pb, name), copy=True)
            fn(a)
            keep.append(a)
            setattr(cb, name, a.ctypes.data)
        return edit

    def null(name):
        return lambda cb, keep: setattr(cb, name, None)

    def first(a):
        a[0] = 1

    def down(a):
        a[len(a) // 2] = a[len(a) // 2 + 1] + 1

    def last_block(a):
        a[-1] = n

    def last_key(a):
        a[-1] = pb.n_keys

    def no_sigs(cb, keep):
        cb.sig_off = cb.sig_text = cb.r_be = cb.s_be = None

    def many(cb, keep):
        cb.n_blocks = 2**32 + 1

    cases = [(null("index"), "null"), (null("hash_off"), "null"), (null("item_block"), "null"),
             (null("key_off"), "key_off"), (swap("hash_off", first), "hash_off[0]"),
             (swap("hash_off", down), "hash_off not monotone"), (swap("tx_start", down), "tx_start"),
             (swap("tx_off", first), "tx_off[0]"), (swap("tx_off", down), "tx_off not monotone"),
             (swap("itx_off", down), "fragment"), (swap("rcpt_off", first), "fragment"),
             (swap("key_off", first), "key_off[0]"), (swap("item_block", last_block), "item_block"),
             (swap("item_key", last_key), "item_key"), (many, "2^32"), (no_sigs, "neither"),
             (null("sig_off"), "sig_off"), (swap("sig_off", first), "sig_off[0]"), (swap("sig_off", down), "monotone"),
             (null("sig_text"), "sig_text")]
    for edit, word in cases:
        rc, err = call(edit)
        assert rc == native.BV_E_ARGS and word in err, (word, rc, err)
    check(c, v0.verify_blocks(pb), "valid call after the refused ones")
    # no blocks, no items: BV_OK
    from babble_amd.batch import BlockBatchBuilder

    e = v0.verify_blocks(BlockBatchBuilder().pack())
    assert e.msg_hash.shape == (0, 32) and e.status.size == 0 and e.valid_count.size == 0


def test_bulk_300_blocks_by_100_validators(v0):
    def make():
        c = BC.signed_case(BC.synth_like_bodies(300), 100, 100, seed=90, corrupt=0.01)
        sample = np.sort(random.Random(91).sample(range(c.n_items), 2000))
        d = c.host()
        from babble_amd.batch import PackedBatch
        from oracle import coracle

        sub = PackedBatch(d.msg_bytes, d.msg_off, d.key_bytes, d.key_off, d.item_msg[sample], d.item_key[sample],
                          d.r_be[sample].copy(), d.s_be[sample].copy(), d.pre[sample].copy())
        h, st, _ = coracle.verify_batch(sub.as_dict())
        return c, sample, h, st

    c, sample, h, st = cached("bulk", make)
    assert c.n_items == 30000 and c.fields.n_blocks == 300 and np.array_equal(h, c.digests)
    assert all(len(b.Transactions) == 16 and len(b.Transactions[0]) == 64 for b in c.bodies[:3])
    ref = v0.verify_text(c.text)  # bv_verify_batch_text over the oracle's serialised bodies
    res = v0.verify_blocks(c.fields)
    t = v0.timing()
    assert t["ms_h2d"] > 0 and t["ms_sha256"] > 0, t
    assert np.array_equal(res.msg_hash, c.digests) and np.array_equal(ref.msg_hash, c.digests)
    assert np.array_equal(res.status, ref.status), np.flatnonzero(res.status != ref.status)[:8]
    assert np.array_equal(res.accept_bits, ref.accept_bits)
    assert np.array_equal(res.status[sample], st)
    assert np.array_equal(res.valid_count, np.bincount(c.fields.item_block[res.status == 1], minlength=300))
    assert 29000 < int(res.valid_count.sum()) < 30000 and set(np.unique(res.status).tolist()) == {0, 1}
