"""BV_DEFER_EXC on the device: one batch just above the throughput threshold
(131,072 + 64 + 5 items, 8 signing keys with at least 8,192 items each) that
carries the crafted exception vectors of tests/defer_vectors.py (for the K12
chain and for the key cache's 22-bit chain; each repeated, so that their two
keys reach the K12 rule too) in a C4 corruption mix of ordinary signatures.
Digests, statuses and accept bits equal to the C oracle's through the device
entry (k_verify_g, k_verify_q), the host entry (k_verify_qf, k_verify_gf) and
a key-cache context with every key registered (k_verify_gq).  These are the
smallest shapes that reach the kernels' throughput forms.  That the crafted
vectors do take the second pass is asserted on the CPU build
(tests/test_defer_exc.py)."""
import numpy as np
import pytest

from babble_amd import native, synth
from babble_amd.batch import PackedBatch
from oracle import coracle
from tests import defer_vectors as dv

pytestmark = pytest.mark.gpu

N_ITEMS = 131072 + 64 + 5
REPEAT = 350  # 2 geometries x 12 vectors a key x 350 = 8,400 items on each crafted key

_CACHE = {}


def case():
    """(batch, digests, statuses, bits, first crafted item), built and run
    through the oracle once."""
    if not _CACHE:
        crafted = dv.vectors() + dv.vectors(22, 6)
        n_crafted = len(crafted) * REPEAT
        base = synth.adversarial(N_ITEMS - n_crafted, seed=9, n_creators=6)
        keys = [base.key(k) for k in range(base.n_keys)]
        kidx = {}
        for _, _, pub, _, _ in crafted:
            if pub not in kidx:
                kidx[pub] = len(keys)
                keys.append(pub)
        msgs = [body for _, body, _, _, _ in crafted]
        msg_bytes = np.concatenate([base.msg_bytes, np.frombuffer(b"".join(msgs), np.uint8)]).copy()
        msg_off = np.concatenate([base.msg_off, base.msg_off[-1] + np.cumsum([len(m) for m in msgs], dtype=np.uint64)])
        key_bytes = np.frombuffer(b"".join(keys), np.uint8).copy()
        key_off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
        im = np.tile(base.n_msgs + np.arange(len(crafted), dtype=np.uint32), REPEAT)
        ik = np.tile(np.array([kidx[v[2]] for v in crafted], np.uint32), REPEAT)
        r = np.tile(np.array([list(v[3].to_bytes(32, "big")) for v in crafted], np.uint8), (REPEAT, 1))
        s = np.tile(np.array([list(v[4].to_bytes(32, "big")) for v in crafted], np.uint8), (REPEAT, 1))
        pre = base.pre if base.pre is not None else np.zeros(base.n_items, np.uint8)
        b = PackedBatch(msg_bytes=msg_bytes, msg_off=msg_off.astype(np.uint64), key_bytes=key_bytes, key_off=key_off,
                        item_msg=np.concatenate([base.item_msg, im]).astype(np.uint32),
                        item_key=np.concatenate([base.item_key, ik]).astype(np.uint32),
                        r_be=np.concatenate([base.r_be, r]), s_be=np.concatenate([base.s_be, s]),
                        pre=np.concatenate([pre, np.zeros(n_crafted, np.uint8)]))
        # 8 signing keys with at least 8,192 items each; the mix's malformed keys are further, tiny ones
        per_key = np.bincount(b.item_key, minlength=b.n_keys)
        assert b.n_items == N_ITEMS and int((per_key >= 8192).sum()) == 8 and int(per_key[per_key < 8192].sum()) < 300
        h, st, bits = coracle.verify_batch(b.as_dict())
        assert len(set(st[base.n_items:base.n_items + len(crafted)].tolist())) >= 1
        assert 0 < int((st == 1).sum()) < N_ITEMS
        _CACHE["case"] = (b, h, st, bits, base.n_items)
    return _CACHE["case"]


def check(res, what):
    b, h, st, bits, first = case()
    assert np.array_equal(res.msg_hash, h), f"{what}: digests differ from oracle"
    bad = np.flatnonzero(res.status != st)
    assert bad.size == 0, f"{what}: {bad.size} statuses differ, first {bad[:8]} (crafted from {first}): " \
                          f"gpu {res.status[bad[:8]]} want {st[bad[:8]]}"
    assert np.array_equal(res.accept_bits, bits), f"{what}: accept bits differ"


def test_device_entry():
    from babble_amd.verifier import Verifier

    b = case()[0]
    v = Verifier(device=0)
    try:
        d = v.to_device(b)
        v.verify_device(d)
        check(d.result(), "device entry")
        assert v.timing()["key_path"] == 12
    finally:
        v.close()


@pytest.mark.parametrize("qfirst", ["1", "0"])
def test_host_entry(monkeypatch, qfirst):
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_QFIRST", qfirst)  # read at bv_create
    b = case()[0]
    v = Verifier(device=0)
    try:
        check(v.verify(b), f"host entry qfirst={qfirst}")
        assert v.timing()["key_path"] == 12
    finally:
        v.close()


def test_key_cache_context():
    from babble_amd.verifier import Verifier

    b = case()[0]
    v = Verifier(device=0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys([b.key(k) for k in range(b.n_keys)])
        check(v.verify(b), "key cache")
        t = v.timing()
        assert t["key_path"] == 22 and t["kc_hits"] >= 8
    finally:
        v.close()
