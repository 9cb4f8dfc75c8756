"""bv_group_verify_events on the GPU: events from their wire fields, sharded
by event index across the group's device slots.  Every group here is made of
logical shards of device 0 (one ctx each): the shard plan, the concurrent
per-shard staging threads, the rebased kernels (k_ev_body_hash_rb,
k_sig_decode_rb) and the shifted bit merge are the multi-device code path,
only the gather is device copies instead of one RCCL all-gather.  The C oracle
over the generator's / the Go-semantics oracle's bodies is the judge."""
import random

import numpy as np
import pytest

from babble_amd import events as E
from babble_amd import native, synth
from tests.test_events import random_wire

pytestmark = pytest.mark.gpu

ACCEPT = native.ACCEPT


def _flipped(n, seed, n_creators=8):
    """A signed bulk batch (parents by hash) with ~1 % of the s values
    corrupted, its wire form, the corrupted rows and the oracle's verdict."""
    from oracle import coracle

    packed, wire = synth.event_fields(n, n_creators=n_creators, seed=seed, parents="hash")
    bad = np.random.default_rng(seed).choice(n, size=max(1, n // 100), replace=False)
    wire.s_be[bad, 5] ^= 0x20
    packed.s_be[bad, 5] ^= 0x20
    return packed, wire, bad, coracle.verify_batch(packed.as_dict())


def _equal(res, want, what=""):
    h, st, bits = want
    assert np.array_equal(res.msg_hash, h), what
    assert np.array_equal(res.status, st), (what, np.flatnonzero(res.status != st)[:8])
    assert np.array_equal(res.accept_bits, bits), what


def test_group_events_match_oracle_and_single_context():
    from babble_amd.verifier import Group, Verifier

    n = 20_011
    packed, wire, bad, want = _flipped(n, 31)
    g = Group([0, 0, 0])
    v = Verifier(0)
    try:
        res = g.verify_events(wire)
        _equal(res, want)
        assert int((res.status != ACCEPT).sum()) == len(bad)
        one = v.verify_events(wire)  # a second witness: the un-based kernels on one context
        _equal(res, (one.msg_hash, one.status, one.accept_bits), "single context")
    finally:
        g.close()
        v.close()


def test_group_events_edge_bodies_across_shards_and_chunks(monkeypatch):
    """nil / empty transaction lists, nil transactions, ITX and BlockSignature
    fragments through shard bounds (384, 768) and 256-event chunk bounds."""
    from babble_amd.batch import PackedBatch
    from babble_amd.verifier import Group
    from oracle import coracle

    monkeypatch.setenv("BV_EV_CHUNK_MB", "0.001")  # 256-event chunks (read at bv_create)
    g = Group([0, 0, 0])
    try:
        for seed in (6, 7):
            wire, bodies, wd = random_wire(seed, n=1100, in_batch=False)
            res = g.verify_events(wire)
            assert [d.tobytes() for d in res.msg_hash] == wd
            n = wire.n_events
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum([len(x) for x in bodies])
            packed = PackedBatch(np.frombuffer(b"".join(bodies), np.uint8).copy(), off, wire.key_bytes,
                                 wire.key_off, np.arange(n, dtype=np.uint32), wire.creator.astype(np.uint32),
                                 wire.r_be, wire.s_be,
                                 wire.pre if wire.pre is not None else np.zeros(n, np.uint8))
            h, st, bits = coracle.verify_batch(packed.as_dict())
            assert np.array_equal(res.status, st) and np.array_equal(res.accept_bits, bits)
    finally:
        g.close()


def test_group_events_empty_and_tiny_shards():
    from babble_amd.verifier import Group, VerifyResult

    g = Group([0, 0, 0])
    try:
        for n in (1, 64, 100, 130):  # shards of (1, 0, 0), (64, 0, 0), (64, 36, 0), (64, 64, 2) events
            packed, wire, bad, want = _flipped(n, 40 + n, n_creators=3)
            res = g.verify_events(wire)
            _equal(res, want, n)
            assert int((res.status != ACCEPT).sum()) == len(bad)
        empty = E.EventBatchBuilder().pack()
        out = VerifyResult(np.full((1, 32), 0xAA, np.uint8), np.full(1, 0xAA, np.uint8),
                           np.full(1, 0xAAAA, np.uint64))
        g.verify_events_into(empty, out)  # BV_OK, nothing written
        assert np.all(out.msg_hash == 0xAA) and out.status[0] == 0xAA and out.accept_bits[0] == 0xAAAA
        assert len(g.verify_events(empty).status) == 0
    finally:
        g.close()


def test_group_events_signature_text():
    """Signature TEXT decoded on the device per shard (k_sig_decode_rb reads
    the shard's slice of the text through the whole batch's offsets)."""
    from babble_amd.verifier import Group
    from oracle import coracle
    from tests.cabi import harness
    from tests.test_hostfuzz import _sig_cases

    n = 3000
    packed, wire, _, _ = _flipped(n, 31)
    text, off = harness.encode_signatures(wire.r_be, wire.s_be)
    sigs = [harness.signature_text(text, off, i) for i in range(n)]
    rng = random.Random(n)
    corpus = _sig_cases(random.Random(7))
    for i in rng.sample(range(n), 40):
        sigs[i] = rng.choice(corpus)
    dec = [native.decode_signature(s) for s in sigs]
    packed.pre = np.array([d[0] for d in dec], np.uint8)
    packed.r_be = np.frombuffer(b"".join(d[1] for d in dec), np.uint8).reshape(n, 32).copy()
    packed.s_be = np.frombuffer(b"".join(d[2] for d in dec), np.uint8).reshape(n, 32).copy()
    want = coracle.verify_batch(packed.as_dict())
    toff = np.zeros(n + 1, np.uint64)
    toff[1:] = np.cumsum([len(x) for x in sigs])
    twire = wire.with_signature_text(np.frombuffer(b"".join(sigs), np.uint8).copy(), toff)
    g = Group([0, 0, 0])
    try:
        _equal(g.verify_events(twire), want)
        assert len(set(np.unique(want[1]).tolist())) >= 2
    finally:
        g.close()


def test_group_events_dag_batch_stays_on_slot_0():
    from babble_amd.verifier import Group
    from oracle import coracle

    packed, wire = synth.event_fields(1000, n_creators=4, seed=12, parents="event")
    g = Group([0, 0])
    try:
        res = g.verify_events(wire)
        h, st, bits = coracle.verify_batch(packed.as_dict())
        assert np.array_equal(res.msg_hash, h) and np.all(res.status == ACCEPT)
        assert np.array_equal(res.accept_bits, bits)
        _, fwd = synth.event_fields(10, n_creators=2, seed=13)
        fwd.parent_kind[3, 0] = E.PARENT_EVENT
        fwd.parent_ref[3, 0] = 5
        with pytest.raises(native.BvError):
            g.verify_events(fwd)
        _equal(g.verify_events(wire), (h, st, bits), "after the refused batch")
    finally:
        g.close()


def test_group_events_pinned_in_place():
    from babble_amd.verifier import Group, PinnedArena, VerifyResult

    n = 5000
    packed, wire, bad, want = _flipped(n, 23)
    g = Group([0, 0])
    arena = PinnedArena()
    try:
        res = VerifyResult(arena.array((n, 32), np.uint8), arena.array(n, np.uint8),
                           arena.array((n + 63) // 64, np.uint64))
        g.verify_events_into(arena.wire(wire), res)
        _equal(res, want)
    finally:
        g.close()
        arena.close()


def test_group_events_key_cache_and_registration():
    from babble_amd.verifier import Group

    n = 6000
    packed, wire, bad, want = _flipped(n, 52, n_creators=3)
    ko = np.asarray(wire.key_off, np.int64)
    keys = [wire.key_bytes[ko[k]:ko[k + 1]].tobytes() for k in range(3)]
    g = Group([0, 0], flags=native.F_KEY_CACHE)
    plain = Group([0, 0])
    try:
        g.register_keys(keys)
        res = g.verify_events(wire)
        for slot in (0, 1):
            t = g.timing(slot)
            assert t["key_path"] == 22 and t["kc_hits"] == 3, (slot, t)
        _equal(res, want)
        with pytest.raises(native.BvError):
            plain.register_keys(keys)
    finally:
        g.close()
        plain.close()
