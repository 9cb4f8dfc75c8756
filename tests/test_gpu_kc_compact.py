"""The compact key-cache tier (BV_F_KEY_CACHE | BV_F_KC_COMPACT: KC18 tables,
18-bit signed windows x 8, 67.1 MB per key) on the GPU, through the C ABI.
The judges are the C oracle and the edge vectors' Python-integer statuses
(tests/edge_vectors_kc18.py), never the library itself.  Every case asserts
the key path it ran (bv_timing.key_path == 18), so a routing change cannot
empty it.  What the vectors offer to the 18 x 8 windows is asserted on the CPU
by tests/test_kc_compact.py.
Run on the GPU box:
    python -u -m pytest tests/test_gpu_kc_compact.py -m gpu -x -v
"""
import numpy as np
import pytest

from babble_amd import native, synth
from oracle import coracle
from oracle import gosemantics as gs
from tests import edge_vectors_kc18 as kv

pytestmark = pytest.mark.gpu

COMPACT = native.F_KEY_CACHE | native.F_KC_COMPACT
LAT_MAX_ITEMS = 131072  # kernels.hip BV_LAT_MAX_ITEMS: larger batches take the throughput point ops
MIX = dict(rflip=20000, sflip=20000, body=10000, highs=10000, range=8000, fmt=8000, key=12000)

_ORACLE = {}


def oracle(name, make):
    """(batch, digests, statuses, bits, tags) of a named vector batch: built,
    run through the C oracle and held to the Python-integer statuses, once."""
    if name not in _ORACLE:
        b, idx = make()
        h, st, bits = coracle.verify_batch(b.as_dict())
        direct = kv.direct_statuses()[idx]
        bad = np.flatnonzero(st != direct)
        assert bad.size == 0, f"oracle differs from Python integers at {bad[:8]}"
        _ORACLE[name] = (b, h, st, bits, [kv.vectors()[i].tag for i in idx])
    return _ORACLE[name]


def whole():
    return oracle("whole", lambda: (kv.batch(), np.arange(len(kv.vectors()))))


def tiled():
    n = len(kv.vectors())
    rep = LAT_MAX_ITEMS // n + 1
    return oracle("tiled", lambda: (kv.batch(repeat=rep), np.tile(np.arange(n), rep)))


def check(res, h, st, bits, tags, what):
    assert np.array_equal(res.msg_hash, h), f"{what}: digests differ from oracle"
    bad = np.flatnonzero(res.status != st)
    assert bad.size == 0, (f"{what}: {bad.size} statuses differ: "
                           + ", ".join(f"{tags[i]} gpu {res.status[i]} want {st[i]}" for i in bad[:12]))
    assert np.array_equal(res.accept_bits, bits), f"{what}: accept bits differ"


def oracle_check(res, b):
    h, st, bits = coracle.verify_batch(b.as_dict())
    assert np.array_equal(res.msg_hash, h), "digests differ from oracle"
    bad = np.flatnonzero(res.status != st)
    assert bad.size == 0, f"{bad.size} statuses differ, first {bad[:8]}: gpu {res.status[bad[:8]]} oracle {st[bad[:8]]}"
    assert np.array_equal(res.accept_bits, bits)
    return st


def valid_keys(b):
    return [b.key(k) for k in range(b.n_keys) if gs.Unmarshal(b.key(k)) is not None]


def wire_keys(wire):
    ko = np.asarray(wire.key_off, np.int64)
    return [wire.key_bytes[ko[k]:ko[k + 1]].tobytes() for k in range(len(ko) - 1)]


# 1 -------------------------------------------------------------------------
def test_edge_vectors_bulk_path(monkeypatch):
    """Every KC18 edge vector (86 keys, 5.8 GB of tables) with all keys
    registered and k_small off: the host entry (k_verify_qf<18, 8> then
    k_verify_gf), the device entry (the fused k_verify_gq<18, 8>), and both
    again tiled just past 131,072 items (the throughput instantiations with
    the pipelined lookups)."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    b, h, st, bits, tags = whole()
    assert 80 <= b.n_keys <= 90 and b.n_items == len(kv.vectors())
    v = Verifier(device=0, flags=COMPACT)
    try:
        v.register_keys([b.key(k) for k in range(b.n_keys)])
        t = v.timing()
        assert t["kc_builds"] == b.n_keys == t["kc_keys"], t
        check(v.verify(b), h, st, bits, tags, "KC18 host entry")
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_hits"] == b.n_keys and t["kc_builds"] == 0, t
        d = v.to_device(b)
        v.verify_device(d)
        check(d.result(), h, st, bits, tags, "KC18 device entry")
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_hits"] == b.n_keys, t
        tb, th, tst, tbits, ttags = tiled()
        n = len(kv.vectors())
        assert LAT_MAX_ITEMS < tb.n_items <= LAT_MAX_ITEMS + n
        assert np.array_equal(tst, np.tile(kv.direct_statuses(), tb.n_items // n))
        check(v.verify(tb), th, tst, tbits, ttags, "KC18 host entry, throughput")
        assert v.timing()["key_path"] == 18
        d = v.to_device(tb)
        v.verify_device(d)
        check(d.result(), th, tst, tbits, ttags, "KC18 device entry, throughput")
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_hits"] == b.n_keys and t["kc_builds"] == 0, t
    finally:
        v.close()


# 2 -------------------------------------------------------------------------
def test_admission_cold_then_warm():
    """An unregistered valid key gets a KC18 table once it has been seen in 2
    batches: per-batch tables first, then a table per distinct valid key,
    then all hits."""
    from babble_amd.verifier import Verifier

    b = synth.adversarial(30_000, seed=41, n_creators=6, scale_per_million=MIX)
    n_valid = len(set(valid_keys(b)))
    assert 0 < n_valid < b.n_keys
    v = Verifier(device=0, flags=COMPACT)
    try:
        st = oracle_check(v.verify(b), b)
        assert set(np.unique(st)) == {0, 1, 2, 3}
        t = v.timing()
        assert t["key_path"] in (8, 12) and t["kc_builds"] == 0, t
        oracle_check(v.verify(b), b)
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_builds"] == n_valid and t["kc_hits"] == 0, t
        oracle_check(v.verify(b), b)
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_builds"] == 0 and t["kc_hits"] == n_valid, t
    finally:
        v.close()


# 3 -------------------------------------------------------------------------
def test_more_keys_than_the_22_bit_tier_holds():
    """150 creators at the default budget (the 805 MB tables stop at 119):
    every key gets a table, the batch and the same events from their wire
    fields run on them, exact."""
    from babble_amd.verifier import Verifier

    packed, wire = synth.event_fields(30_000, n_creators=150, seed=71, parents="hash")
    bad = np.random.default_rng(71).choice(packed.n_items, size=300, replace=False)
    wire.s_be = np.asarray(wire.s_be).copy()
    wire.s_be[bad, 5] ^= 0x20
    packed.s_be[bad, 5] ^= 0x20
    h, st, bits = coracle.verify_batch(packed.as_dict())
    assert int((st != native.ACCEPT).sum()) == len(bad)
    keys = wire_keys(wire)
    assert len(set(keys)) == 150 == packed.n_keys
    v = Verifier(device=0, flags=COMPACT)
    try:
        v.register_keys(keys)
        t = v.timing()
        assert t["kc_builds"] == 150 and t["kc_keys"] == 150, t
        res = v.verify(packed)
        assert np.array_equal(res.msg_hash, h) and np.array_equal(res.status, st)
        assert np.array_equal(res.accept_bits, bits)
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_hits"] == 150 and t["kc_builds"] == 0, t
        res = v.verify_events(wire)
        assert np.array_equal(res.msg_hash, h) and np.array_equal(res.status, st)
        assert np.array_equal(res.accept_bits, bits)
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_hits"] == 150, t
    finally:
        v.close()


# 4 -------------------------------------------------------------------------
def test_budget_and_eviction(monkeypatch):
    """0.25 GB holds 3 tables of 67,108,928 bytes.  Registering 5 keys builds
    the first 3; a batch naming all 5 takes the per-batch tables.  Without
    registration, 2 new keys after 2 others evict the least recently used."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_KEY_CACHE_GB", "0.25")
    monkeypatch.setenv("BV_KC_ADMIT", "1")
    b = synth.adversarial(20_000, seed=46, n_creators=5, scale_per_million=MIX)
    assert len(set(valid_keys(b))) == 5
    v = Verifier(device=0, flags=COMPACT)
    try:
        v.register_keys([b.key(k) for k in range(b.n_keys)])
        t = v.timing()
        assert t["kc_builds"] == 3 and t["kc_keys"] == 3, t
        for _ in range(2):
            oracle_check(v.verify(b), b)
            t = v.timing()
            assert t["key_path"] in (8, 12) and t["kc_keys"] == 3 and t["kc_builds"] == 0, t
    finally:
        v.close()
    v = Verifier(device=0, flags=COMPACT)
    try:
        a = synth.events(3000, n_creators=2, seed=51)
        c = synth.events(3000, n_creators=2, seed=52)
        oracle_check(v.verify(a), a)
        t = v.timing()
        assert t["kc_builds"] == 2 and t["key_path"] == 18, t
        oracle_check(v.verify(c), c)
        t = v.timing()
        assert t["kc_builds"] == 2 and t["kc_keys"] <= 3 and t["key_path"] == 18, t
        oracle_check(v.verify(a), a)
        t = v.timing()
        assert t["kc_keys"] <= 3 and t["key_path"] == 18, t
    finally:
        v.close()


# 5 -------------------------------------------------------------------------
def test_small_batches_on_a_compact_context():
    """k_small reads no KC18 tables: batches of 1 and 100 items of registered
    creators run it as for keys without a table (key_path 0, no hits); the
    1000-item batch takes the bulk pipeline on the tables."""
    from babble_amd.verifier import Verifier

    v = Verifier(device=0, flags=COMPACT)
    try:
        for n in (1, 100, 1000):
            b = synth.events(n, n_creators=4, seed=100 + n)
            v.register_keys([b.key(k) for k in range(b.n_keys)])
            assert v.timing()["kc_builds"] == b.n_keys
            oracle_check(v.verify(b), b)
            t = v.timing()
            if n == 1000:
                assert t["key_path"] == 18 and t["kc_hits"] == b.n_keys and t["kc_builds"] == 0, t
            else:
                assert t["key_path"] == 0 and t["kc_hits"] == 0 and t["kc_builds"] == 0, (n, t)
    finally:
        v.close()


# 6 -------------------------------------------------------------------------
def test_failure_leaves_no_unbuilt_slot(monkeypatch):
    """The 3rd table allocation of a 64-key miss batch fails: the call takes
    the per-batch path with nothing indexed, the next builds every table."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_KC_ADMIT", "1")
    monkeypatch.setenv("BV_KC_FAIL", "alloc:3")
    b = synth.adversarial(40_000, seed=44, n_creators=64, scale_per_million=MIX)
    n_valid = len(set(valid_keys(b)))
    v = Verifier(device=0, flags=COMPACT)
    try:
        oracle_check(v.verify(b), b)
        t = v.timing()
        assert t["key_path"] in (8, 12) and t["kc_keys"] == 0 and t["kc_builds"] == 0, t
        oracle_check(v.verify(b), b)
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_builds"] == n_valid and t["kc_keys"] == n_valid, t
        d = v.to_device(b)
        v.verify_device(d)
        oracle_check(d.result(), b)
        t = v.timing()
        assert t["kc_hits"] == n_valid and t["kc_builds"] == 0 and t["key_path"] == 18, t
    finally:
        v.close()


# 7 -------------------------------------------------------------------------
def test_partial_mode(monkeypatch):
    """BV_KC_PARTIAL=1: one fresh valid key among 19 registered ones keeps the
    cache; its items are left deferred by the KC18 kernels and finished by
    the generic path."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_KC_ADMIT", "1000")
    monkeypatch.setenv("BV_KC_PARTIAL", "1")
    b = synth.events(30_000, n_creators=20, seed=62)
    rng = np.random.default_rng(62)
    for i in rng.choice(b.n_items, 300, replace=False):
        b.r_be[i, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
    keys = [b.key(k) for k in range(b.n_keys)]
    v = Verifier(device=0, flags=COMPACT)
    try:
        v.register_keys(keys[1:])
        for device_api in (False, True):
            if device_api:
                d = v.to_device(b)
                v.verify_device(d)
                res = d.result()
            else:
                res = v.verify(b)
            st = oracle_check(res, b)
            assert int((st == native.ACCEPT).sum()) == b.n_items - 300
            t = v.timing()
            assert t["key_path"] == 18 and t["kc_hits"] == 19 and t["kc_builds"] == 0, (device_api, t)
    finally:
        v.close()


# 8 -------------------------------------------------------------------------
def test_group():
    """Two logical shards of device 0, each a compact context: registration,
    a packed batch and the same events from their wire fields."""
    from babble_amd.verifier import Group

    packed, wire = synth.event_fields(4000, n_creators=5, seed=83, parents="hash")
    bad = np.random.default_rng(83).choice(packed.n_items, size=40, replace=False)
    wire.s_be = np.asarray(wire.s_be).copy()
    wire.s_be[bad, 5] ^= 0x20
    packed.s_be[bad, 5] ^= 0x20
    h, st, bits = coracle.verify_batch(packed.as_dict())
    assert int((st != native.ACCEPT).sum()) == len(bad)
    g = Group([0, 0], flags=COMPACT)
    try:
        g.register_keys(wire_keys(wire))
        res = g.verify(packed)
        assert np.array_equal(res.msg_hash, h) and np.array_equal(res.status, st)
        assert np.array_equal(res.accept_bits, bits)
        for slot in (0, 1):
            t = g.timing(slot)
            assert t["key_path"] == 18 and t["kc_hits"] == 5, (slot, t)
        res = g.verify_events(wire)
        assert np.array_equal(res.msg_hash, h) and np.array_equal(res.status, st)
        assert np.array_equal(res.accept_bits, bits)
        for slot in (0, 1):
            t = g.timing(slot)
            assert t["key_path"] == 18 and t["kc_hits"] == 5, (slot, t)
    finally:
        g.close()
