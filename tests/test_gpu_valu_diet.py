"""The instruction-count cuts of the throughput step through the real
kernels: the GLV split in plain integers (field.h BV_GLV_INT: k_glv_split,
item_scalars, verify_item_qfirst, the key-cache kernel) and the K12 sub-tables
from shared multiples (verify_core.h BV_FILL_SHARED: k_fill_multiples,
k_table_fill_shared).  Digests, statuses and accept bits equal to the C
oracle's, exactly.

One batch serves the three cases: 131,072 + 64 + 5 items — the smallest size
that takes the throughput kernels (batches <= 131,072 items take the latency
variants), with a ragged last bitmask word — from 8 creators with the C4
corruption mix, and the key-cache subset of the chosen-scalar edge vectors
(tests/edge_vectors.py: empty and extreme GLV halves, x(R) >= N, exceptional
totals) spliced in mid-wave, messages and items at the same position so that
items stay in message order.  Every case asserts the key path it ran.
Run on the GPU box:
    python -u -m pytest tests/test_gpu_valu_diet.py -m gpu -x -v
"""
import numpy as np
import pytest

from babble_amd import native, synth
from babble_amd.batch import PackedBatch
from oracle import coracle
from oracle import gosemantics as gs
from tests import edge_vectors as ev

pytestmark = pytest.mark.gpu

N_ITEMS = 131_072 + 64 + 5
SPLICE_AT = 70_001
MIX = dict(rflip=20000, sflip=20000, body=10000, highs=10000, range=8000, fmt=8000, key=12000)

_CASE = {}


def splice(base, extra, p):
    """`extra`'s messages, keys and items inserted into `base` at message /
    item position p (base has one message per item, in order)."""
    assert np.array_equal(base.item_msg, np.arange(base.n_items, dtype=np.uint32))
    m = extra.n_msgs
    cut = int(base.msg_off[p])
    msg_bytes = np.concatenate([base.msg_bytes[:cut], extra.msg_bytes, base.msg_bytes[cut:]])
    msg_off = np.concatenate([base.msg_off[:p], extra.msg_off[:-1] + np.uint64(cut),
                              base.msg_off[p:] + np.uint64(len(extra.msg_bytes))]).astype(np.uint64)
    key_bytes = np.concatenate([base.key_bytes, extra.key_bytes])
    key_off = np.concatenate([base.key_off, extra.key_off[1:] + base.key_off[-1]]).astype(np.uint64)

    def cat(a, b):
        return np.concatenate([a[:p], b, a[p:]])

    item_msg = cat(base.item_msg, extra.item_msg + np.uint32(p)).astype(np.uint32)
    item_msg[p + extra.n_items:] += np.uint32(m)
    item_key = cat(base.item_key, extra.item_key + np.uint32(base.n_keys)).astype(np.uint32)
    pre_b = base.pre if base.pre is not None else np.zeros(base.n_items, np.uint8)
    pre_e = extra.pre if extra.pre is not None else np.zeros(extra.n_items, np.uint8)
    return PackedBatch(msg_bytes, msg_off, key_bytes, key_off, item_msg, item_key, cat(base.r_be, extra.r_be),
                       cat(base.s_be, extra.s_be), cat(pre_b, pre_e))


def case():
    """(batch, digests, statuses, bits, good keys): built, and run through the
    C oracle, once for the module."""
    if not _CASE:
        idx = ev.kc_subset()
        extra = ev.batch(idx)
        base = synth.adversarial(N_ITEMS - extra.n_items, seed=81, n_creators=8, scale_per_million=MIX)
        b = splice(base, extra, SPLICE_AT)
        assert b.n_items == N_ITEMS and b.n_items % 64 != 0 and SPLICE_AT % 64 != 0
        assert np.all(np.diff(b.item_msg.astype(np.int64)) >= 0)
        h, st, bits = coracle.verify_batch(b.as_dict())
        edge = st[SPLICE_AT:SPLICE_AT + len(idx)]
        assert np.array_equal(edge, ev.direct_statuses()[idx]), "oracle differs from Python integers on the edge vectors"
        assert set(np.unique(st)) == {0, 1, 2, 3}
        good = sorted({b.key(k) for k in range(b.n_keys) if gs.Unmarshal(b.key(k)) is not None})
        _CASE["x"] = (b, h, st, bits, good)
    return _CASE["x"]


def check(res, h, st, bits, what):
    assert np.array_equal(res.msg_hash, h), f"{what}: digests differ from oracle"
    bad = np.flatnonzero(res.status != st)
    assert bad.size == 0, f"{what}: {bad.size} statuses differ, first {bad[:8]}: gpu {res.status[bad[:8]]} want {st[bad[:8]]}"
    assert np.array_equal(res.accept_bits, bits), f"{what}: accept bits differ"


def env(monkeypatch):
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")  # read at bv_create
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")


def test_device_entry(monkeypatch):
    """(a) Inputs resident in HBM: k_glv_split on the s^-1 stream, the K12
    tables by k_fill_multiples / k_table_fill_shared / k_table_pair beside it,
    k_verify_g<false, true> and k_verify_q<12, 11, false>."""
    from babble_amd.verifier import Verifier

    env(monkeypatch)
    b, h, st, bits, _ = case()
    v = Verifier(device=0)
    try:
        d = v.to_device(b)
        v.verify_device(d)
        check(d.result(), h, st, bits, "device entry")
        assert v.timing()["key_path"] == 12
    finally:
        v.close()


def test_host_entry(monkeypatch):
    """(b) The same batch from host memory: k_verify_qf (the split inside
    verify_item_qfirst) over the batch, then k_verify_gf per hashed chunk."""
    from babble_amd.verifier import Verifier

    env(monkeypatch)
    b, h, st, bits, _ = case()
    v = Verifier(device=0)
    try:
        check(v.verify(b), h, st, bits, "host entry")
        assert v.timing()["key_path"] == 12
    finally:
        v.close()


def test_key_cache(monkeypatch):
    """(c) The same batch with every valid key registered: the fused
    key-cache kernel k_verify_gq forms u1, u2 and the split itself."""
    from babble_amd.verifier import Verifier

    env(monkeypatch)
    b, h, st, bits, good = case()
    assert len(good) <= 48
    v = Verifier(device=0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys(good)
        d = v.to_device(b)
        v.verify_device(d)
        check(d.result(), h, st, bits, "key cache")
        t = v.timing()
        assert t["key_path"] == 22 and t["kc_hits"] == len(good)
    finally:
        v.close()
