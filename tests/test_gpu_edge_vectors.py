"""The chosen-scalar edge vectors (tests/edge_vectors.py) through every verify
path of the real kernels: digests, statuses and accept bits equal to the C
oracle's, and statuses equal to the Python-integer verification.  What the
vectors offer to each path (every window / digit-class pair of the generator,
K12, K8 and KC tables, the cold scheduler's NAF patterns, the final check's
wrap and guard cases) is asserted on the CPU by tests/test_edge_vectors.py.
Every case asserts the key path it ran, so a routing change cannot empty it.
Run on the GPU box:
    python -u -m pytest tests/test_gpu_edge_vectors.py -m gpu -x -v
"""
import numpy as np
import pytest

from babble_amd import native, shard
from oracle import coracle
from tests import edge_vectors as ev
from tests.helpers import bits_from_status

pytestmark = pytest.mark.gpu

LAT_MAX_ITEMS = 131072  # kernels.hip BV_LAT_MAX_ITEMS: larger batches take the throughput point ops

_ORACLE = {}


def oracle(name, make):
    """(batch, digests, statuses, bits, tags) of a named batch: built, and run
    through the C oracle, once for the module."""
    if name not in _ORACLE:
        b, idx = make()
        h, st, bits = coracle.verify_batch(b.as_dict())
        direct = ev.direct_statuses()[idx]
        bad = np.flatnonzero(st != direct)
        assert bad.size == 0, f"oracle differs from Python integers at {bad[:8]}"
        _ORACLE[name] = (b, h, st, bits, [ev.vectors()[i].tag for i in idx])
    return _ORACLE[name]


def whole():
    return oracle("whole", lambda: (ev.batch(), np.arange(len(ev.vectors()))))


def kc():
    return oracle("kc", lambda: (ev.batch(ev.kc_subset()), np.array(ev.kc_subset())))


def tiled():
    n = len(ev.vectors())
    rep = LAT_MAX_ITEMS // n + 1
    return oracle("tiled", lambda: (ev.batch(repeat=rep), np.tile(np.arange(n), rep)))


def check(res, h, st, bits, tags, what):
    """check_against_oracle's three comparisons (tests/test_gpu.py), naming
    the vectors that differ."""
    assert np.array_equal(res.msg_hash, h), f"{what}: digests differ from oracle"
    bad = np.flatnonzero(res.status != st)
    assert bad.size == 0, (f"{what}: {bad.size} statuses differ: "
                           + ", ".join(f"{tags[i]} gpu {res.status[i]} want {st[i]}" for i in bad[:12]))
    assert np.array_equal(res.accept_bits, bits), f"{what}: accept bits differ"


def check_slices(v, cuts, key_path, what, other=None):
    """The whole batch in item slices [lo, hi): each against the oracle's
    rows, and item for item against a second verifier when given."""
    b, h, st, bits, tags = whole()
    for lo, hi in cuts:
        s = shard.slice_batch(b, lo, hi)
        res = v.verify(s)
        check(res, h[lo:hi], st[lo:hi], bits_from_status(st[lo:hi]), tags[lo:hi], f"{what} [{lo}, {hi})")
        assert v.timing()["key_path"] == key_path, (what, lo, hi)
        if other is not None:
            ref = other.verify(s)
            assert np.array_equal(ref.status, res.status) and np.array_equal(ref.msg_hash, res.msg_hash), (what, lo, hi)


def cuts_of(n, sizes):
    out, lo, k = [], 0, 0
    while lo < n:
        hi = min(n, lo + sizes[k % len(sizes)])
        out.append((lo, hi))
        lo, k = hi, k + 1
    return out


def test_generic_per_lane_path(monkeypatch):
    """One item per key, more than 256 keys, k_small off: the per-lane
    Strauss-Shamir path (and the 26-bit generator windows with R entering as
    k1 Q + k2 phi(Q))."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    b, h, st, bits, tags = whole()
    assert b.n_keys > 256 and b.n_items < 8 * b.n_keys
    v = Verifier(device=0)
    try:
        check(v.verify(b), h, st, bits, tags, "generic")
        assert v.timing()["key_path"] == 0
    finally:
        v.close()


@pytest.mark.parametrize("qfirst", ["1", "0"])
@pytest.mark.parametrize("w", [8, 12])
def test_per_batch_key_tables(monkeypatch, w, qfirst):
    """K8 (BV_F_K8) and K12 per-batch tables built for every vector's key,
    through the host entry with the key part first (k_verify_qf, then
    k_verify_gf: key_table_add's from-identity window, g_table_add on a
    non-identity R) and with u1 G first (g_table_add's FROM_INF, then
    k_verify_q)."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_QFIRST", qfirst)
    b, h, st, bits, tags = whole()
    v = Verifier(device=0, flags=native.F_K8 if w == 8 else native.F_DEFAULT)
    try:
        check(v.verify(b), h, st, bits, tags, f"K{w} qfirst={qfirst}")
        assert v.timing()["key_path"] == w
    finally:
        v.close()


def test_k12_device_entry(monkeypatch):
    """The device entry (inputs in HBM, the GLV split on the s^-1 stream by
    k_glv_split) with K12 tables."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    b, h, st, bits, tags = whole()
    v = Verifier(device=0)
    try:
        d = v.to_device(b)
        v.verify_device(d)
        check(d.result(), h, st, bits, tags, "K12 device entry")
        assert v.timing()["key_path"] == 12
    finally:
        v.close()


def test_small_kernel_cold_path():
    """k_small without key tables (the NAF digits of k1 / k2 scheduled into
    barrier-separated phases; the G leaves by table_leaf) in slices of 256,
    37 and 5 items."""
    from babble_amd.verifier import Verifier

    v = Verifier(device=0)
    try:
        check_slices(v, cuts_of(len(ev.vectors()), (256, 37, 5)), 0, "k_small cold")
    finally:
        v.close()


def test_small_kernel_host_item_records(monkeypatch):
    """Slices of 1 to 4 items carry host item records (hostscalar.h: u1 and
    the GLV split computed on the host); the same slices with
    BV_HOST_SCALARS=0 compute them on the device: equal to the oracle and to
    each other, item for item."""
    from babble_amd.verifier import Verifier

    n = len(ev.vectors())
    rng = np.random.default_rng(78)
    cuts = cuts_of(n, [int(x) for x in rng.integers(1, 5, size=n)])
    rec = Verifier(device=0)
    monkeypatch.setenv("BV_HOST_SCALARS", "0")  # read at bv_create
    dev = Verifier(device=0)
    try:
        check_slices(rec, cuts, 0, "k_small records", other=dev)
    finally:
        rec.close()
        dev.close()


def test_key_cache_bulk_path(monkeypatch):
    """The KC subset (families d and e, the KC rotations; 32 keys) with every
    key registered and k_small off: the fused key-cache kernel (22-bit signed
    windows, phi(T) formed per lookup)."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    b, h, st, bits, tags = kc()
    assert b.n_keys <= 32
    v = Verifier(device=0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys([b.key(k) for k in range(b.n_keys)])
        check(v.verify(b), h, st, bits, tags, "KC bulk")
        t = v.timing()
        assert t["key_path"] == 22 and t["kc_hits"] == b.n_keys
    finally:
        v.close()


def test_small_kernel_warm_with_kc_tables():
    """The KC subset through k_small with every key's table cached (22 table
    leaves and the sum tree), whole and in slices of up to 16 items (host
    item records)."""
    from babble_amd.verifier import Verifier

    b, h, st, bits, tags = kc()
    v = Verifier(device=0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys([b.key(k) for k in range(b.n_keys)])
        check(v.verify(b), h, st, bits, tags, "k_small warm")
        t = v.timing()
        assert t["key_path"] == 22 and t["kc_hits"] == b.n_keys and t["ms_h2d"] == 0  # k_small: no staging copy
        for lo, hi in cuts_of(b.n_items, (16, 9, 5, 13)):
            s = shard.slice_batch(b, lo, hi)
            res = v.verify(s)
            check(res, h[lo:hi], st[lo:hi], bits_from_status(st[lo:hi]), tags[lo:hi],
                  f"k_small warm records [{lo}, {hi})")
            assert v.timing()["key_path"] == 22
    finally:
        v.close()


@pytest.mark.parametrize("w", [12, 8])
def test_throughput_point_op_variants(monkeypatch, w):
    """Every vector repeated as further items on its message and key until
    the batch is just past 131,072 items: the verify kernels' throughput
    variants, K12 and K8.  The expected statuses are the base statuses tiled;
    the oracle runs on the tiled batch once."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")  # read at bv_create
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    b, h, st, bits, tags = tiled()
    n = len(ev.vectors())
    assert LAT_MAX_ITEMS < b.n_items <= LAT_MAX_ITEMS + n
    assert np.array_equal(st, np.tile(ev.direct_statuses(), b.n_items // n))
    v = Verifier(device=0, flags=native.F_K8 if w == 8 else native.F_DEFAULT)
    try:
        check(v.verify(b), h, st, bits, tags, f"K{w} throughput")
        assert v.timing()["key_path"] == w
    finally:
        v.close()
