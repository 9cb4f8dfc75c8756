"""The digest edge vectors of tests/digest_vectors.py through the real kernels
and the library's own dispatch, the digests supplied by the test
(tests/chaincheck, with the runners, sizes and knobs of
tests/test_gpu_chain_exceptions.py): e = 0 and e = N (u1 = 0: the generator
chain never leaves the identity, and every later stage takes an identity
accumulator), e >= N up to 2^256 - 1 (the digest is read unreduced), limb
patterns of e, a generator half empty over a whole wave's range of k_small's
warm tree, and the REJECT twins — a stage that loses the identity flag ends on
X = ZZ = 0, which final_check accepts for any r, so only the twins show it.

Statuses are compared exactly with the vectors' expected ones, which
tests/test_digest_vectors.py holds equal to oracle.gosemantics.item_status,
the C oracle and OpenSSL over the same digests; run_bulk also checks that the
digests come back unchanged, the accept bits, and the key path each case ran.
All 71 vectors and one plain valid vector per key, tiled to the size, in
every case:
  * K12 and K8 in device order (k_verify_g: g_table_add<FROM_INF> stays at
    the identity, rg_store / rg_load carry inf = 1; k_verify_q's key_table_add
    starts from it), KC22 and KC18 bulk (k_verify_gq), the generic path
    (k_verify_generic), each at the latency size and at 131,072 + 64 + 5 items;
  * the host-entry order (k_verify_qf, then k_verify_gf adding nothing onto
    R_Q: its FINAL top window has d == 0) for K12, K8, KC22 and KC18, both
    sizes, in chunks, and once with BV_QFIRST=0;
  * k_small cold (wave 3 joins an identity G sum; with k2 = 0 too, acc3 is
    handed over as the identity) and warm on KC22 and KC18 (wave 0's whole
    range is identity nodes, which reach the 4 -> 2 level), the device forming
    the scalars and over host item records.
The generic path and k_small have no host build: this is the only execution
of these vectors through them."""
import pytest

from babble_amd import native
from tests import digest_vectors as dg
from tests.test_gpu_chain_exceptions import ENDS, SIZES, run_bulk, run_small, with_fillers

pytestmark = pytest.mark.gpu

SIZE_VALUES = [p.values[0] for p in SIZES]  # the latency and the throughput size, as they are


def batch():
    """every vector, and one plain valid vector on each of the two keys"""
    vecs = with_fillers(dg.vectors())
    assert len(vecs) == dg.N_VECTORS + 2 and len({v.pub for v in vecs}) == 2
    return vecs


@pytest.mark.parametrize("geom", ["K12", "K8"])
def test_per_batch_tables_device_order(monkeypatch, geom):
    """k_verify_g then k_verify_q<12 | 8>, the latency and the throughput
    (alternating-Y) instantiations on one context."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    v = Verifier(device=0, flags=native.F_K8 if geom == "K8" else native.F_DEFAULT)
    try:
        for n_items in SIZE_VALUES:
            run_bulk(v, batch(), n_items, 12 if geom == "K12" else 8, f"digest {geom} {n_items}")
    finally:
        v.close()


@pytest.mark.parametrize("geom", ["KC22", "KC18"])
def test_key_cache_bulk(monkeypatch, geom):
    """k_verify_gq<22 | 18> with both keys registered, both sizes."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    vecs = batch()
    v = Verifier(device=0, flags=native.F_KEY_CACHE | (native.F_KC_COMPACT if geom == "KC18" else 0))
    try:
        v.register_keys(sorted({x.pub for x in vecs}))
        for n_items in SIZE_VALUES:
            run_bulk(v, vecs, n_items, 22 if geom == "KC22" else 18, f"digest {geom} {n_items}")
            assert v.timing()["kc_hits"] == 2
    finally:
        v.close()


def test_generic_path(monkeypatch):
    """k_verify_generic (no key table): u2 Q whole, then generator windows
    that are all zero digits for u1 = 0; both sizes."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1000000")
    monkeypatch.setenv("BV_LAT_TABLE_KEYS", "0")
    v = Verifier(device=0)
    try:
        for n_items in SIZE_VALUES:
            run_bulk(v, batch(), n_items, 0, f"digest generic {n_items}")
    finally:
        v.close()


@pytest.mark.parametrize("geom", ["K12", "K8"])
def test_per_batch_tables_host_order(monkeypatch, geom):
    """k_verify_qf<12 | 8> from the identity, then k_verify_gf onto R_Q, the
    items in chunks; both sizes."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    v = Verifier(device=0, flags=native.F_K8 if geom == "K8" else native.F_DEFAULT)
    try:
        for n_items in SIZE_VALUES:
            run_bulk(v, batch(), n_items, 12 if geom == "K12" else 8, f"digest host order {geom} {n_items}",
                     ends=ENDS[n_items])
    finally:
        v.close()


@pytest.mark.parametrize("geom", ["KC22", "KC18"])
def test_key_cache_host_order(monkeypatch, geom):
    """k_verify_qf<22 | 18> over the two keys' cached tables, then
    k_verify_gf; both sizes."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    vecs = batch()
    v = Verifier(device=0, flags=native.F_KEY_CACHE | (native.F_KC_COMPACT if geom == "KC18" else 0))
    try:
        v.register_keys(sorted({x.pub for x in vecs}))
        for n_items in SIZE_VALUES:
            run_bulk(v, vecs, n_items, 22 if geom == "KC22" else 18, f"digest host order {geom} {n_items}",
                     ends=ENDS[n_items])
            assert v.timing()["kc_hits"] == 2
    finally:
        v.close()


def test_host_order_entry_without_qfirst(monkeypatch):
    """BV_QFIRST=0: no key part first (k_verify_g + k_verify_q chunk by
    chunk), the same statuses."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create
    monkeypatch.setenv("BV_TABLE_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_K12_MIN_ITEMS", "1")
    monkeypatch.setenv("BV_QFIRST", "0")
    v = Verifier(device=0)
    try:
        run_bulk(v, batch(), 300, 12, "digest host order K12 300, BV_QFIRST=0", ends=ENDS[300], qf=False)
    finally:
        v.close()


@pytest.mark.parametrize("records", [False, True], ids=["device-scalars", "host-records"])
def test_small_kernel_cold_path(monkeypatch, records):
    """k_small without a table: wave 3 joins an identity G sum at kColdGJoin
    (u1 = 0), and where k2 = 0 as well hands over an identity acc3; the
    device forming the scalars (cc_verify_small) and over host item records
    (cc_verify_small_rec, 4 items a launch)."""
    from babble_amd.verifier import Verifier

    monkeypatch.delenv("BV_HOST_SCALARS", raising=False)  # read at bv_create
    v = Verifier(device=0)
    try:
        run_small(v, batch(), False, f"digest k_small cold, records={records}", records=records)
    finally:
        v.close()


@pytest.mark.parametrize("geom", ["KC22", "KC18"])
def test_small_kernel_warm_tree(monkeypatch, geom):
    """k_small's warm tree over cached tables (built by one bulk call
    first): for u1 = 0 all five generator pairs are identity nodes, so wave
    0's whole range is, and the identity reaches the 4 -> 2 level; the g/
    vectors empty wave 0's range with u1 != 0.  The device forming the
    scalars, then over host item records, on one context."""
    from babble_amd.verifier import Verifier

    monkeypatch.setenv("BV_SMALL", "0")  # read at bv_create (the warm-up bulk call)
    monkeypatch.delenv("BV_HOST_SCALARS", raising=False)
    vecs = batch()
    v = Verifier(device=0, flags=native.F_KEY_CACHE | (native.F_KC_COMPACT if geom == "KC18" else 0))
    try:
        if geom == "KC18":
            v.kc_small_tables(True)
        v.register_keys(sorted({x.pub for x in vecs}))
        run_bulk(v, vecs, len(vecs), 22 if geom == "KC22" else 18, f"digest warm-up {geom}")  # builds the tables
        for records in (False, True):
            hits, n_keys = run_small(v, vecs, True, f"digest k_small warm {geom}, records={records}", records=records)
            assert hits == n_keys == 2
    finally:
        v.close()
