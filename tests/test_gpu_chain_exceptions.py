"""Valid signatures whose addition chains meet an exceptional addition
(tests/chain_vectors.py), through the real kernels and the library's own
dispatch with the digests supplied by the test (tests/chaincheck): a doubling
or a P + (-P) that gives a wrong point turns an ACCEPT into a REJECT here,
which the hashed-message vectors of tests/test_gpu_defer_exc.py cannot show.
Statuses are compared exactly with chain_vectors' expected ones (ACCEPT,
except the vectors whose total is the identity), which
tests/test_chain_exceptions.py holds equal to oracle.gosemantics.item_status
over the same digests; the digests that come back must be the ones sent in,
and every case asserts the key path it ran.

Bulk entry (cc_verify_bulk: verify_device_impl with `hashed` digests), each at
a latency size (a few hundred items, the path forced with the knobs of
tests/test_gpu_edge_vectors.py) and at 131,072 + 64 + 5 items (the throughput
forms; the crafted vectors tiled with a plain valid vector per key):
K12 and K8 in device order (k_verify_g, k_verify_q), KC22 and KC18
(k_verify_gq), the generic path (k_verify_generic).
Small entry (cc_verify_small: one k_small launch, the device forming every
scalar): the cold path and the warm tree for KC22 and KC18 tables.

The two orders a host caller takes, over the same sizes and knobs:
the host-entry order (cc_verify_hostorder: bv_host_launch's call sequence,
k_verify_qf summing R_Q from the identity, then k_verify_gf adding the
generator windows onto it in three or four chunks, so with lo > 0 and a ragged
last word) for K12, K8, KC22 and KC18 with chain_vectors.host_vectors, whose
R_Q meets a generator window, and host_invalid_twins, the same chains under
signatures that must REJECT; and k_small over host item records
(cc_verify_small_rec: bv_host_item_records' u1, k1, k2 in mapped host memory,
as many items a launch as bv_small_verify would give records) with the cold
and warm vectors."""
import ctypes
import os

import numpy as np
import pytest

from babble_amd import native
from tests import chain_vectors as cv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "chaincheck", "libchaincheck.so")
N_ITEMS = 131072 + 64 + 5  # tests/test_gpu_defer_exc.py's size: just past the latency variants' limit
_LIB = []


def lib():
    if not _LIB:
        if not os.path.exists(LIB):
            pytest.fail("tests/chaincheck/libchaincheck.so missing: run __graft_entry__.build()")
        native.lib()  # the product library first: chaincheck links it
        L = ctypes.CDLL(LIB)
        V = ctypes.c_void_p
        L.cc_verify_bulk.argtypes = [V, V, V, V]
        L.cc_verify_bulk.restype = ctypes.c_int
        L.cc_verify_small.argtypes = [V, ctypes.c_uint32, ctypes.c_uint32] + [V] * 7 + [ctypes.c_int, V, V, V, V]
        L.cc_verify_small.restype = ctypes.c_int
        L.cc_verify_hostorder.argtypes = [V, V, V, V, ctypes.c_uint32, V, V]
        L.cc_verify_hostorder.restype = ctypes.c_int
        L.cc_verify_small_rec.argtypes = ([V, ctypes.c_uint32, ctypes.c_uint32] + [V] * 7 + [ctypes.c_int] + [V] * 7
                                          + [V, V, V])
        L.cc_verify_small_rec.restype = ctypes.c_int
        _LIB.append(L)
    return _LIB[0]


def bits_of(st):
    pad = (-len(st)) % 64
    return np.packbits(np.concatenate([st == 1, np.zeros(pad, bool)]), bitorder="little").view(np.uint64)


def run_bulk(v, vecs, n_items, key_path, what, ends=None, qf=True):
    """vecs tiled to n_items items through cc_verify_bulk on verifier v, or,
    with `ends` (the chunk ends), through cc_verify_hostorder, which must
    report the key part first exactly when `qf`."""
    import torch

    rep = -(-n_items // len(vecs))
    b, dig, want = cv.batch(vecs, rep)
    b, want = _head(b, n_items), want[:n_items]
    d = v.to_device(b)
    ddig = torch.from_numpy(dig.reshape(-1)).to(torch.device("cuda", v.device))
    torch.cuda.synchronize(v.device)
    if ends is None:
        rc = lib().cc_verify_bulk(v._ctx, ctypes.addressof(d.cbatch), ctypes.addressof(d.cresult), ddig.data_ptr())
    else:
        assert len(ends) >= 2 and 0 < ends[0] and ends[-1] < n_items and n_items % 64  # >= 3 chunks, a ragged last word
        e = np.array(ends, np.uint64)
        ran_qf = ctypes.c_int(-1)
        rc = lib().cc_verify_hostorder(v._ctx, ctypes.addressof(d.cbatch), ctypes.addressof(d.cresult),
                                       ddig.data_ptr(), len(e), e.ctypes.data, ctypes.addressof(ran_qf))
    assert rc == 0, (what, rc, native.lib().bv_last_error(v._ctx))
    if ends is not None:  # else the run silently took the device order
        assert ran_qf.value == (1 if qf else 0), (what, "key part first:", ran_qf.value)
    res = d.result()
    assert np.array_equal(res.msg_hash, dig), f"{what}: the digests changed"
    bad = np.flatnonzero(res.status != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {n_items} statuses differ: "
                           + ", ".join(f"{vecs[i % len(vecs)].tag} gpu {res.status[i]} want {want[i]}"
                                       for i in bad[:12]))
    assert np.array_equal(res.accept_bits, bits_of(want)), f"{what}: accept bits differ"
    assert v.timing()["key_path"] == key_path, (what, v.timing()["key_path"])


def _head(b, n):
    from babble_amd.batch import PackedBatch

    return PackedBatch(msg_bytes=b.msg_bytes, msg_off=b.msg_off, key_bytes=b.key_bytes, key_off=b.key_off,
                       item_msg=b.item_msg[:n].copy(), item_key=b.item_key[:n].copy(), r_be=b.r_be[:n].copy(),
                       s_be=b.s_be[:n].copy(), pre=b.pre[:n].copy() if b.pre is not None else None)


def with_fillers(vecs):
    """the crafted vectors and one plain valid vector on each of their keys"""
    keys = []
    for v in vecs:
        if v.c not in keys:
            keys.append(v.c)
    return vecs + [cv.plain(0xF111 + i, 1, c)[0] for i, c in enumerate(keys)]


SIZES = [pytest.param(300, id="latency"), pytest.param(N_ITEMS, id="throughput")]


@pytest.mark.parametrize("n_items", SIZES)
@pytest.mark.parametrize("geom", ["K12", "K8"])
def test_per_batch_tables_device_order(monkeypatch, geom, n_items):
    """k_verify_g then k_verify_q<12 | 8>: 24 vectors whose key chain meets
    the first, a middle and the last non-zero window of either GLV half as a
    doubling and as P + (-P) (22 ACCEPT; the 2 that end on the identity
    REJECT), the latency (LAT) and the throughput (alternating-Y)
    instantiations."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    v = Verifier(device=0, flags=native.F_K8 if geom == "K8" else native.F_DEFAULT)
    try:
        run_bulk(v, with_fillers(cv.k_vectors(geom)), n_items, 12 if geom == "K12" else 8, f"{geom} {n_items}")
    finally:
        v.close()


@pytest.mark.parametrize("n_items", SIZES)
@pytest.mark.parametrize("geom", ["KC22", "KC18"])
def test_key_cache_bulk(monkeypatch, geom, n_items):
    """k_verify_gq<22 | 18> with both keys registered: the same 24 targets on
    the cached geometry's chain (phi(T) formed per lookup)."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    vecs = with_fillers(cv.k_vectors(geom))
    v = Verifier(device=0, flags=native.F_KEY_CACHE | (native.F_KC_COMPACT if geom == "KC18" else 0))
    try:
        v.register_keys(sorted({x.pub for x in vecs}))
        run_bulk(v, vecs, n_items, 22 if geom == "KC22" else 18, f"{geom} {n_items}")
        assert v.timing()["kc_hits"] == 2
    finally:
        v.close()


@pytest.mark.parametrize("n_items", SIZES)
def test_generic_path(monkeypatch, n_items):
    """k_verify_generic (no key table: BV_TABLE_MIN_ITEMS out of reach and no
    latency tables): u2 Q is whole when the generator windows are added, and
    12 vectors (each on its own key) meet the first, a middle and the last
    non-zero generator window both ways (10 ACCEPT, 2 REJECT): g_table_add on
    a Jacobian accumulator, gej_add_ge / gej_add_ge_lat's doubling branch."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1000000")
    monkeypatch.setenv("BV_LAT_TABLE_KEYS", "0")
    v = Verifier(device=0)
    try:
        run_bulk(v, with_fillers(cv.generic_vectors()), n_items, 0, f"generic {n_items}")
    finally:
        v.close()


def host_batch():
    """host_vectors and, on the same chains, their twins that do not verify
    (REJECT where a mishandled exceptional addition could leave a state that
    final_check accepts)"""
    return cv.host_vectors() + cv.host_invalid_twins()


# chunk ends of the host-order runs: k_verify_gf with lo == 0, lo > 0, and a ragged last word at the end
ENDS = {300: [64, 256], N_ITEMS: [64, 4096, 65600]}


@pytest.mark.parametrize("n_items", SIZES)
@pytest.mark.parametrize("geom", ["K12", "K8"])
def test_per_batch_tables_host_order(monkeypatch, geom, n_items):
    """k_verify_qf<12 | 8> from the identity, then k_verify_gf onto R_Q: 12
    vectors whose R_Q meets the first, a middle and the last (the FINAL,
    xz_only) non-zero generator window as a doubling and as P + (-P) (10
    ACCEPT; the 2 that end on the identity REJECT) and their 12 invalid twins
    (REJECT), the latency and the throughput instantiations, the items in
    chunks."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    v = Verifier(device=0, flags=native.F_K8 if geom == "K8" else native.F_DEFAULT)
    try:
        run_bulk(v, with_fillers(host_batch()), n_items, 12 if geom == "K12" else 8, f"host order {geom} {n_items}",
                 ends=ENDS[n_items])
    finally:
        v.close()


@pytest.mark.parametrize("n_items", SIZES)
@pytest.mark.parametrize("geom", ["KC22", "KC18"])
def test_key_cache_host_order(monkeypatch, geom, n_items):
    """k_verify_qf<22 | 18> over the two keys' cached tables (phi(T) formed
    per lookup), then k_verify_gf: the same 12 vectors and twins."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    vecs = with_fillers(host_batch())
    v = Verifier(device=0, flags=native.F_KEY_CACHE | (native.F_KC_COMPACT if geom == "KC18" else 0))
    try:
        v.register_keys(sorted({x.pub for x in vecs}))
        run_bulk(v, vecs, n_items, 22 if geom == "KC22" else 18, f"host order {geom} {n_items}", ends=ENDS[n_items])
        assert v.timing()["kc_hits"] == 2
    finally:
        v.close()


def test_host_order_entry_without_qfirst(monkeypatch):
    """BV_QFIRST=0: the same call reports that no key part ran first (the
    pipe runs k_verify_g + k_verify_q chunk by chunk) and the statuses are the
    expected ones all the same."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_QFIRST", "0")
    v = Verifier(device=0)
    try:
        run_bulk(v, with_fillers(host_batch()), 300, 12, "host order K12 300, BV_QFIRST=0", ends=ENDS[300], qf=False)
    finally:
        v.close()


def run_small(v, vecs, kc, what, records=False):
    """one k_small launch over the vectors (one item, one digest each); with
    `records`, k_small over host item records, in as many launches as the
    product's limit on records makes it"""
    import torch

    dev = torch.device("cuda", v.device)
    b, dig, want = cv.batch(vecs)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    kb = np.concatenate([b.key_bytes, np.zeros(64, np.uint8)])
    ko = b.key_off.astype(np.uint64)
    bufs = [t(dig), t(kb), t(ko), t(b.item_msg.astype(np.uint32)), t(b.item_key.astype(np.uint32)), t(b.r_be),
            t(b.s_be)]
    st = torch.full((b.n_items,), 0xEE, dtype=torch.uint8, device=dev)
    hits = ctypes.c_uint32(0)
    torch.cuda.synchronize(v.device)
    if records:
        host = [np.ascontiguousarray(dig), np.ascontiguousarray(b.item_msg, np.uint32),
                np.ascontiguousarray(b.item_key, np.uint32), np.ascontiguousarray(b.r_be), np.ascontiguousarray(b.s_be)]
        launches = ctypes.c_uint32(0)
        rc = lib().cc_verify_small_rec(v._ctx, b.n_items, b.n_keys, *[x.data_ptr() for x in bufs], 1 if kc else 0,
                                       kb.ctypes.data, ko.ctypes.data, *[x.ctypes.data for x in host], st.data_ptr(),
                                       ctypes.addressof(hits), ctypes.addressof(launches))
        assert rc == 0, (what, rc, native.lib().bv_last_error(v._ctx))
        per = 16 if kc else 4  # bv_ctx::host_scalar_max's default; without tables the product stops at 4
        assert launches.value == -(-b.n_items // per), (what, launches.value)
    else:
        rc = lib().cc_verify_small(v._ctx, b.n_items, b.n_keys, *[x.data_ptr() for x in bufs], 1 if kc else 0,
                                   b.key_bytes.ctypes.data, ko.ctypes.data, st.data_ptr(), ctypes.addressof(hits))
    assert rc == 0, (what, rc, native.lib().bv_last_error(v._ctx))
    got = st.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: " + ", ".join(f"{vecs[i].tag} gpu {got[i]} want {want[i]}" for i in bad[:12])
    return hits.value, b.n_keys


def test_small_kernel_cold_path():
    """k_small without a table, 18 vectors and 2 plain ones: wave 3's chain
    (the G sum, then +-phi(2^i Q)) meeting the first, a middle and the last
    NAF digit of k2 both ways; the final k1 Q + acc3 as a doubling; acc3
    handed over as the identity (ACCEPT, R = k1 Q); the identity total
    (REJECT) — coop::add_xyzz's branches and cold_add_node's identity flag."""
    from babble_amd.verifier import Verifier

    v = Verifier(device=0)
    try:
        run_small(v, with_fillers(cv.cold_vectors()), False, "k_small cold")
    finally:
        v.close()


@pytest.mark.parametrize("geom", ["KC22", "KC18"])
def test_small_kernel_warm_tree(monkeypatch, geom):
    """k_small's warm tree over cached tables (each vector's key registered
    and its table built by one bulk call first): the cross-chain nodes of
    coop_sum_nodes — generator pairs meeting the first k1 pairs inside wave
    1's range, the 4 -> 2 level, the root — as doublings and as P + (-P), and
    two vectors whose leaf pairs are both zero digits (identity nodes)."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create (the warm-up bulk call)
    vecs = cv.warm_vectors(geom)
    v = Verifier(device=0, flags=native.F_KEY_CACHE | (native.F_KC_COMPACT if geom == "KC18" else 0))
    try:
        if geom == "KC18":
            v.kc_small_tables(True)
        v.register_keys(sorted({x.pub for x in vecs}))
        run_bulk(v, vecs, len(vecs), 22 if geom == "KC22" else 18, f"warm-up {geom}")  # builds the tables
        hits, n_keys = run_small(v, vecs, True, f"k_small warm {geom}")
        assert hits == n_keys == len({x.pub for x in vecs})
    finally:
        v.close()


def test_small_kernel_cold_path_host_records(monkeypatch):
    """k_small's rec != NULL form without a table, as bv_small_verify runs
    every batch of up to 4 items: the cold vectors and fillers, 4 items a
    launch, u1 and the GLV halves from bv_host_item_records, the key decoded
    from the record — the same chains and targets as the cold-path test."""
    from babble_amd.verifier import Verifier

    monkeypatch.delenv("BV_HOST_SCALARS", raising=False)  # read at bv_create
    v = Verifier(device=0)
    try:
        run_small(v, with_fillers(cv.cold_vectors()), False, "k_small cold, records", records=True)
    finally:
        v.close()


@pytest.mark.parametrize("geom", ["KC22", "KC18"])
def test_small_kernel_warm_tree_host_records(monkeypatch, geom):
    """k_small's rec != NULL form over cached tables (the table address in
    the record), up to host_scalar_max items a launch: the warm tree's
    vectors, after the same warm-up bulk call as the rec == NULL test."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create (the warm-up bulk call)
    monkeypatch.delenv("BV_HOST_SCALARS", raising=False)
    vecs = cv.warm_vectors(geom)
    v = Verifier(device=0, flags=native.F_KEY_CACHE | (native.F_KC_COMPACT if geom == "KC18" else 0))
    try:
        if geom == "KC18":
            v.kc_small_tables(True)
        v.register_keys(sorted({x.pub for x in vecs}))
        run_bulk(v, vecs, len(vecs), 22 if geom == "KC22" else 18, f"warm-up {geom}")  # builds the tables
        hits, n_keys = run_small(v, vecs, True, f"k_small warm {geom}, records", records=True)
        assert hits == n_keys == len({x.pub for x in vecs})
    finally:
        v.close()
