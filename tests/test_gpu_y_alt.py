"""BV_Y_ALT on the device: one batch just above the throughput threshold
(131,072 + 64 + 5 items, 8 signing keys with at least 8,192 items each) that
carries the crafted vectors of tests/test_y_alt.py — the doubling and inverse
vectors of tests/defer_vectors.py (for the K12 chain and for the key cache's
22-bit chain; each repeated, so that their two keys reach the K12 rule too)
and, on the same two keys (the K12 rule allows the batch no more), the
zero-window vectors of tests/yalt_vectors.py (shared_key_vectors, for the
device's 26-bit generator windows with K12 and with the key cache's
geometry) — in a C4 corruption mix of ordinary signatures.  Digests, statuses
and accept bits equal to the C oracle's through the device entry (k_verify_g,
k_verify_q), the host entry in both orders (k_verify_qf, k_verify_gf) and a
key-cache context with every key registered (k_verify_gq).

With the key fixed those zero-window signatures cannot be made to verify, so
the last two cases tile the ones that do (yalt_vectors.vectors: every one an
ACCEPT by construction, each on a key of its own, so a wrong sign in the chain
shows as a REJECT) to the same size, with a K12 table for every key and with
every key in a key cache: the skip fix-up of the generator chain and of both
halves of the key chain at window 0, an even, an odd, two consecutive and the
last window.  That the vectors do reach those paths is asserted on the CPU
build (tests/test_y_alt.py)."""
import numpy as np
import pytest

from babble_amd import native, synth
from babble_amd.batch import PackedBatch
from oracle import coracle
from tests import defer_vectors as dv
from tests import yalt_vectors as yv

pytestmark = pytest.mark.gpu

N_ITEMS = 131072 + 64 + 5
REPEAT = 350  # 2 geometries x 12 vectors a key x 350 = 8,400 items on each crafted key
GW, GNWIN = 26, 10  # the device's generator-table geometry

_CACHE = {}


def _append(base, vecs, reps):
    """base followed by every vector of vecs[g] reps[g] times (group after
    group, a group's vectors in turn)."""
    keys = [base.key(k) for k in range(base.n_keys)]
    kidx = {}
    msgs, im, ik, r, s = [], [], [], [], []
    for vec, rep in zip(vecs, reps):
        first = base.n_msgs + len(msgs)
        for _, body, pub, _, _ in vec:
            if pub not in kidx:
                kidx[pub] = len(keys)
                keys.append(pub)
            msgs.append(body)
        im.append(np.tile(first + np.arange(len(vec), dtype=np.uint32), rep))
        ik.append(np.tile(np.array([kidx[v[2]] for v in vec], np.uint32), rep))
        r.append(np.tile(np.array([list(v[3].to_bytes(32, "big")) for v in vec], np.uint8), (rep, 1)))
        s.append(np.tile(np.array([list(v[4].to_bytes(32, "big")) for v in vec], np.uint8), (rep, 1)))
    n_new = sum(len(x) for x in im)
    msg_bytes = np.concatenate([base.msg_bytes, np.frombuffer(b"".join(msgs), np.uint8)]).copy()
    msg_off = np.concatenate([base.msg_off, base.msg_off[-1] + np.cumsum([len(m) for m in msgs], dtype=np.uint64)])
    key_bytes = np.frombuffer(b"".join(keys), np.uint8).copy()
    key_off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
    pre = base.pre if base.pre is not None else np.zeros(base.n_items, np.uint8)
    return PackedBatch(msg_bytes=msg_bytes, msg_off=msg_off.astype(np.uint64), key_bytes=key_bytes, key_off=key_off,
                       item_msg=np.concatenate([base.item_msg] + im).astype(np.uint32),
                       item_key=np.concatenate([base.item_key] + ik).astype(np.uint32),
                       r_be=np.concatenate([base.r_be] + r), s_be=np.concatenate([base.s_be] + s),
                       pre=np.concatenate([pre, np.zeros(n_new, np.uint8)]))


def case():
    """(batch, digests, statuses, bits, first crafted item), built and run
    through the oracle once."""
    if "case" not in _CACHE:
        crafted = dv.vectors() + dv.vectors(22, 6)
        zero = yv.shared_key_vectors(GW, GNWIN) + yv.shared_key_vectors(GW, GNWIN, 22, 6)
        n_extra = len(crafted) * REPEAT + len(zero)
        base = synth.adversarial(N_ITEMS - n_extra, seed=11, n_creators=6)
        b = _append(base, [crafted, zero], [REPEAT, 1])
        # 8 signing keys with at least 8,192 items each; the mix's malformed keys are further, tiny ones
        per_key = np.bincount(b.item_key, minlength=b.n_keys)
        assert b.n_items == N_ITEMS and int((per_key >= 8192).sum()) == 8 and int(per_key[per_key < 8192].sum()) < 300
        h, st, bits = coracle.verify_batch(b.as_dict())
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


@pytest.mark.parametrize("path", ["k12", "kc"])
def test_zero_window_vectors_tiled(monkeypatch, path):
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")  # read at bv_create: a K12 table for every key
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    zero = yv.vectors(GW, GNWIN) if path == "k12" else yv.vectors(GW, GNWIN, 22, 6)
    rep = N_ITEMS // len(zero) + 1
    b = _append(synth.adversarial(64, seed=12, n_creators=2), [zero], [rep])
    assert b.n_items > 131072 and b.n_keys <= 32
    h, st, bits = coracle.verify_batch(b.as_dict())
    assert (st[64:] == 1).all()
    v = Verifier(device=0, flags=native.F_KEY_CACHE if path == "kc" else native.F_DEFAULT)
    try:
        if path == "kc":
            v.register_keys([b.key(k) for k in range(b.n_keys)])
        d = v.to_device(b)
        v.verify_device(d)
        res = d.result()
        bad = np.flatnonzero(res.status != st)
        assert bad.size == 0, f"{bad.size} statuses differ: {sorted({zero[(i - 64) % len(zero)][0] for i in bad if i >= 64})}"
        assert np.array_equal(res.msg_hash, h) and np.array_equal(res.accept_bits, bits)
        assert v.timing()["key_path"] == (12 if path == "k12" else 22)
    finally:
        v.close()
