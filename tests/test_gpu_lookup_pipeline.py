"""The throughput verify kernels' pipelined table lookups (verify_core.h
entry_stage: window j+1's entry requested into LDS before window j's
addition), the trimmed last addition and the folded GLV-half sign, through
the device entry: digests, statuses and accept bits equal to the C oracle's.
131,072 is BV_LAT_MAX_ITEMS; only larger batches reach the changed loops.
Every case asserts the key path it ran.
Run on the GPU box:
    python -u -m pytest tests/test_gpu_lookup_pipeline.py -m gpu -x -v
"""
import numpy as np
import pytest

from babble_amd import native, synth
from oracle import coracle
from tests import edge_vectors as ev
from tests import test_gpu_edge_vectors as tev

pytestmark = pytest.mark.gpu

LAT_MAX_ITEMS = tev.LAT_MAX_ITEMS
SMOKE_MIX = dict(rflip=20000, sflip=20000, body=10000, highs=10000, range=8000, fmt=8000, key=12000)  # smoke()'s

_ADV = {}


def tiled_kc():
    idx = ev.kc_subset()
    rep = LAT_MAX_ITEMS // len(idx) + 1
    return tev.oracle("tiled_kc", lambda: (ev.batch(idx, repeat=rep), np.tile(np.array(idx), rep)))


def adversarial(seed):
    """(batch, digests, statuses, bits) of smoke()'s mix at 131,072 + 257
    items: no multiple of 64, early-return lanes and working lanes in the
    same waves.  Built and run through the oracle once per seed."""
    if seed not in _ADV:
        b = synth.adversarial(LAT_MAX_ITEMS + 257, seed=seed, scale_per_million=SMOKE_MIX)
        h, st, bits = coracle.verify_batch(b.as_dict())
        counts = np.bincount(st, minlength=4)
        assert counts.min() > 0, counts  # every status among the lanes
        _ADV[seed] = (b, h, st, bits)
    return _ADV[seed]


def env(monkeypatch):
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")  # read at bv_create
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")


@pytest.mark.parametrize("w", [12, 8])
def test_tiled_edge_vectors_device_entry(monkeypatch, w):
    """Every edge vector repeated to just past 131,072 items, inputs resident
    in HBM: k_verify_g<false, true> (g_table_add from the identity) and
    k_verify_q<12 | 8, ., false> (both GLV halves, both signs, the trimmed
    last window)."""
    from babble_amd.verifier import Verifier

    env(monkeypatch)
    b, h, st, bits, tags = tev.tiled()
    assert LAT_MAX_ITEMS < b.n_items
    v = Verifier(device=0, flags=native.F_K8 if w == 8 else native.F_DEFAULT)
    try:
        d = v.to_device(b)
        v.verify_device(d)
        tev.check(d.result(), h, st, bits, tags, f"K{w} device entry, tiled")
        assert v.timing()["key_path"] == w
    finally:
        v.close()


def test_tiled_kc_subset_key_cache_bulk(monkeypatch):
    """The KC subset tiled past 131,072 items with every key registered: the
    fused key-cache kernel's throughput variant (g_table_add, then both
    halves of key_table_add with phi(T) per lookup)."""
    from babble_amd.verifier import Verifier

    env(monkeypatch)
    b, h, st, bits, tags = tiled_kc()
    assert LAT_MAX_ITEMS < b.n_items and b.n_keys <= 32
    v = Verifier(device=0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys([b.key(k) for k in range(b.n_keys)])
        d = v.to_device(b)
        v.verify_device(d)
        tev.check(d.result(), h, st, bits, tags, "KC device entry, tiled")
        t = v.timing()
        assert t["key_path"] == 22 and t["kc_hits"] == b.n_keys
    finally:
        v.close()


def test_adversarial_mix_device_entry(monkeypatch):
    """A staged entry consumed by the wrong lane, or a prefetch issued by a
    lane that has left, shows here: waves mix every status."""
    from babble_amd.verifier import Verifier

    env(monkeypatch)
    b, h, st, bits = adversarial(7)
    assert b.n_items % 64 != 0
    v = Verifier(device=0)
    try:
        d = v.to_device(b)
        v.verify_device(d)
        res = d.result()
        assert np.array_equal(res.msg_hash, h), "digests differ from oracle"
        assert np.array_equal(res.status, st), np.flatnonzero(res.status != st)[:10]
        assert np.array_equal(res.accept_bits, bits), "accept bits differ"
        assert v.timing()["key_path"] == 12
    finally:
        v.close()


def test_two_batches_in_flight(monkeypatch):
    """Two different batches on the context's two work slots, results read
    after one synchronize: each wave's LDS slots are its own."""
    import torch

    from babble_amd.verifier import Verifier

    env(monkeypatch)
    b1, h1, st1, bits1 = adversarial(7)
    b2, h2, st2, bits2 = adversarial(11)
    assert not np.array_equal(st1, st2)
    v = Verifier(device=0)
    try:
        d1, d2 = v.to_device(b1), v.to_device(b2)
        v.verify_device(d1, stream=0, sync=False)  # the library's lane of the call's work slot
        s1 = v.last_stream()
        v.verify_device(d2, stream=0, sync=False)
        assert v.last_stream() != s1, "the two calls ran on one work slot"
        v.sync()
        torch.cuda.synchronize()
        for d, h, st, bits in ((d1, h1, st1, bits1), (d2, h2, st2, bits2)):
            res = d.result()
            assert np.array_equal(res.msg_hash, h), "digests differ from oracle"
            assert np.array_equal(res.status, st), np.flatnonzero(res.status != st)[:10]
            assert np.array_equal(res.accept_bits, bits), "accept bits differ"
    finally:
        v.close()
