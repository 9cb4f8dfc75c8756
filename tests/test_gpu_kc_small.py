"""KC18 tables in the one-launch small-batch kernel (bv_kc_small_tables on a
BV_F_KEY_CACHE | BV_F_KC_COMPACT context: k_small<18, 8>, 10 G leaves + 2 x 8
table leaves) on the GPU, through the C ABI.  The judges are the C oracle and
the edge vectors' Python-integer statuses (tests/edge_vectors_kc18.py), never
the library itself.  Every case asserts the path it ran: key_path 18 with
ms_h2d == 0 is k_small on the tables (the bulk pipeline stages its inputs, so
its ms_h2d is positive; k_small reads them in place).  What the table lanes
address is held to Python integers on the CPU by tests/test_kc_small.py.
Run on the GPU box:
    python -u -m pytest tests/test_gpu_kc_small.py -m gpu -x -v
"""
import numpy as np
import pytest

from babble_amd import native, shard, synth
from babble_amd.batch import PackedBatch
from oracle import coracle
from oracle import gosemantics as gs
from tests import edge_vectors_kc18 as kv
from tests.helpers import bits_from_status

pytestmark = pytest.mark.gpu

COMPACT = native.F_KEY_CACHE | native.F_KC_COMPACT
SMALL_MAX, SMALL_WARM_MAX = 256, 1024  # bv_internal.h small_max / small_warm_max
MIX = dict(rflip=20000, sflip=20000, body=10000, highs=10000, range=8000, fmt=8000, key=12000)
# the same with 3 malformed keys per 1000 items: synth.adversarial deals the
# kinds in order, and the first three (empty, 33-byte compressed, prefix 0x06)
# are malformed by their FORM.  A 65-byte 0x04 key off the curve is a
# well-formed key without a table, and a batch past 256 items that names one is
# not "fully cached".
MIX_FORM_KEYS = dict(MIX, key=3000)

_WHOLE = []


def whole():
    """(batch, digests, statuses, bits, tags) of every KC18 edge vector: run
    through the C oracle and held to the Python-integer statuses, once."""
    if not _WHOLE:
        b = kv.batch()
        h, st, bits = coracle.verify_batch(b.as_dict())
        bad = np.flatnonzero(st != kv.direct_statuses())
        assert bad.size == 0, f"oracle differs from Python integers at {bad[:8]}"
        _WHOLE.append((b, h, st, bits, [v.tag for v in kv.vectors()]))
    return _WHOLE[0]


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


def cuts_of(n, sizes):
    out, lo, k = [], 0, 0
    while lo < n:
        hi = min(n, lo + sizes[k % len(sizes)])
        out.append((lo, hi))
        lo, k = hi, k + 1
    return out


def used_keys_only(b):
    """The batch with the keys no item names dropped from its key table."""
    used, inv = np.unique(b.item_key, return_inverse=True)
    keys = [b.key(int(k)) for k in used]
    off = np.zeros(len(keys) + 1, np.uint64)
    off[1:] = np.cumsum([len(k) for k in keys])
    kb = np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy()
    return PackedBatch(b.msg_bytes, b.msg_off, kb, off, b.item_msg, inv.astype(np.uint32), b.r_be, b.s_be, b.pre)


def creators(b):
    """The distinct valid keys of the batch's key table."""
    return sorted({b.key(k) for k in range(b.n_keys) if gs.Unmarshal(b.key(k)) is not None})


def compact(keys, small_tables=True):
    from babble_amd.verifier import Verifier

    v = Verifier(device=0, flags=COMPACT)
    try:
        v.register_keys(keys)
        t = v.timing()
        assert t["kc_builds"] == len(keys) == t["kc_keys"], t
        if small_tables:
            v.kc_small_tables(True)
    except BaseException:
        v.close()
        raise
    return v


def small_on_tables(t, hits):
    """k_small read KC18 tables: no staging copy, the geometry reported, nothing built."""
    return t["key_path"] == 18 and t["kc_hits"] == hits and t["kc_builds"] == 0 and t["ms_h2d"] == 0


# 1 -------------------------------------------------------------------------
def test_edge_vectors_whole():
    """Every KC18 edge vector in one batch, every key registered: one
    k_small<18, 8> launch, 26 leaves per item."""
    b, h, st, bits, tags = whole()
    assert 80 <= b.n_keys <= 90 and b.n_items == len(kv.vectors())
    assert b.n_items <= SMALL_MAX  # the first size class (the 257-1024 extension: test_synth_sizes)
    v = compact([b.key(k) for k in range(b.n_keys)])
    try:
        check(v.verify(b), h, st, bits, tags, "k_small on KC18 tables")
        t = v.timing()
        assert small_on_tables(t, b.n_keys), t
    finally:
        v.close()


# 2 -------------------------------------------------------------------------
def test_edge_vectors_sliced(monkeypatch):
    """The vectors in slices of up to 16 items (host item records: every
    item's key has a table) and of 1-4 items, and again on a context that
    never uses records (the device inverts s and splits u2 itself)."""
    b, h, st, bits, tags = whole()
    keys = [b.key(k) for k in range(b.n_keys)]
    cuts = cuts_of(b.n_items, (16, 9, 5, 13)) + cuts_of(b.n_items, (1, 2, 3, 4))
    v = compact(keys)
    monkeypatch.setenv("BV_HOST_SCALARS", "0")  # read at bv_create
    w = compact(keys)
    try:
        for lo, hi in cuts:
            s = shard.slice_batch(b, lo, hi)
            want = (h[lo:hi], st[lo:hi], bits_from_status(st[lo:hi]), tags[lo:hi])
            a = v.verify(s)
            check(a, *want, f"records [{lo}, {hi})")
            assert small_on_tables(v.timing(), b.n_keys), (lo, hi, v.timing())
            c = w.verify(s)
            check(c, *want, f"no records [{lo}, {hi})")
            assert small_on_tables(w.timing(), b.n_keys), (lo, hi, w.timing())
            assert np.array_equal(a.status, c.status) and np.array_equal(a.accept_bits, c.accept_bits)
    finally:
        v.close()
        w.close()


# 3 -------------------------------------------------------------------------
def synth_batch(n):
    if n == 1:
        return synth.events(1, n_creators=4, seed=301)  # (too small for the mix)
    if n <= SMALL_MAX:
        return synth.adversarial(n, seed=300 + n, n_creators=4, scale_per_million=MIX)
    return used_keys_only(synth.adversarial(n, seed=300 + n, n_creators=4, scale_per_million=MIX_FORM_KEYS))


@pytest.mark.parametrize("n", [1, 17, 100, 256, 257, 1000])
def test_synth_sizes(n):
    """4 registered creators and the corruption mix at both size classes'
    edges: bad r / s, format errors and malformed keys through the decision
    table, the valid keys' items through the tables."""
    b = synth_batch(n)
    assert b.n_items == n
    if n > SMALL_MAX:  # the 257-1024 extension needs every well-formed key cached
        assert n <= SMALL_WARM_MAX
        assert all(gs.Unmarshal(k) is not None for k in map(b.key, range(b.n_keys)) if len(k) == 65 and k[0] == 4)
        assert any(gs.Unmarshal(b.key(k)) is None for k in range(b.n_keys))
    keys = creators(b)
    assert len(keys) == 4
    v = compact(keys)
    try:
        st = oracle_check(v.verify(b), b)
        if n >= 17:
            assert len(set(np.unique(st))) >= 3, np.unique(st)
        t = v.timing()
        assert small_on_tables(t, 4), (n, t)
        if n == 100:  # <= 4 items always get host records, malformed keys among them
            for lo, hi in cuts_of(n, (4, 3)):
                s = shard.slice_batch(b, lo, hi)
                oracle_check(v.verify(s), s)
                assert small_on_tables(v.timing(), 4), (lo, hi, v.timing())
    finally:
        v.close()


def test_a_well_formed_key_without_a_table_ends_the_extension():
    """1000 items whose key table holds a 65-byte 0x04 key off the curve: not
    fully cached, so the batch takes the bulk pipeline (on the tables)."""
    b = synth.adversarial(1000, seed=1300, n_creators=4, scale_per_million=MIX)
    assert any(len(b.key(k)) == 65 and b.key(k)[0] == 4 and gs.Unmarshal(b.key(k)) is None for k in range(b.n_keys))
    v = compact(creators(b))
    try:
        oracle_check(v.verify(b), b)
        t = v.timing()
        assert t["key_path"] == 18 and t["kc_hits"] == 4 and t["ms_h2d"] > 0, t
    finally:
        v.close()


# 4 -------------------------------------------------------------------------
def test_mixed_warm_and_cold():
    """One valid creator of 5 is not registered: at 100 items its items take
    the doubling chain in the same launch as the others' table leaves; 1000
    items are past the cold limit and not fully cached, so they leave k_small."""
    b = synth.events(100, n_creators=5, seed=401)
    keys = creators(b)
    assert len(keys) == 5 == b.n_keys
    cold = b.key(int(b.item_key[7]))
    n_cold = int(sum(b.key(int(k)) == cold for k in b.item_key))
    assert 0 < n_cold < 100
    v = compact([k for k in keys if k != cold])
    try:
        st = oracle_check(v.verify(b), b)
        assert int((st == native.ACCEPT).sum()) == 100
        t = v.timing()
        assert small_on_tables(t, b.n_keys - 1) and t["kc_keys"] == 4, t
        big = synth.events(1000, n_creators=5, seed=401)
        assert sorted(creators(big)) == keys
        oracle_check(v.verify(big), big)
        t = v.timing()
        assert t["ms_h2d"] > 0, t  # the bulk pipeline's staging copy
    finally:
        v.close()


# 5 -------------------------------------------------------------------------
def test_switching_off_restores_the_routing():
    b = synth.events(100, n_creators=4, seed=501)
    v = compact(creators(b), small_tables=False)
    try:
        for on, path, hits in ((False, 0, 0), (True, 18, 4), (False, 0, 0)):
            v.kc_small_tables(on)
            oracle_check(v.verify(b), b)
            t = v.timing()
            assert (t["key_path"], t["kc_hits"], t["kc_builds"], t["ms_h2d"]) == (path, hits, 0, 0), (on, t)
    finally:
        v.close()


@pytest.mark.parametrize("flags", [native.F_KEY_CACHE, native.F_DEFAULT])
def test_other_contexts_refuse(flags):
    from babble_amd.verifier import Verifier

    v = Verifier(device=0, flags=flags)
    try:
        for on in (True, False):
            with pytest.raises(native.BvError) as e:
                v.kc_small_tables(on)
            assert e.value.code == native.BV_E_ARGS and "BV_F_KC_COMPACT" in str(e.value)
    finally:
        v.close()


def test_22_bit_context_is_unchanged():
    """k_small<22, 6>: a 22-bit context's warm small batches, whole and with records."""
    from babble_amd.verifier import Verifier

    b = synth.adversarial(100, seed=601, n_creators=4, scale_per_million=MIX)
    v = Verifier(device=0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys(creators(b))
        oracle_check(v.verify(b), b)
        t = v.timing()
        assert t["key_path"] == 22 and t["kc_hits"] == 4 and t["ms_h2d"] == 0, t
        s = shard.slice_batch(b, 0, 3)
        oracle_check(v.verify(s), s)
        assert v.timing()["key_path"] == 22
    finally:
        v.close()
