"""The field-boundary keys of tests/key_vectors.py through every path of the
real kernels that decodes a key.  key_decode_point's device body (aligned
dword loads realigned by key_off & 3) is not the host body the emulator
compiles, so the range check and the limb assembly are pinned here: every
status, the accept bits and the key path of every run are compared exactly,
and every vector is in every run.

Forged valid triples (the test supplies the digest: tests/chaincheck) give
ACCEPT under the good key, REF_PANIC under its out-of-range twin and REJECT
under the twin with r = N or s = 0; an ACCEPT under coordinates like p - 3 or
2^256 - 1 - 2^(32 i) also shows that the decoded limbs feed the table
builders.  Items over real bodies with an (r, s) that does not verify (REJECT
under a good key, REF_PANIC under a bad one) go through the public entries in
the four key alignments and with a vector key last in key_bytes.

Call sites of key_decode_point and what reaches them:
  k_key_decode            every bulk run (key_path 12 / 8 / 0 with ms_h2d > 0,
                          18 / 22) and bv_kc_register
  k_small from key_bytes  cc_verify_small; Verifier.verify at 5..256 items
                          (key_path 0, ms_h2d == 0)
  k_small from a record   cc_verify_small_rec (4 items a launch, asserted by
                          run_small); Verifier.verify at <= 4 items
"""
import numpy as np
import pytest

from babble_amd import native, shard
from babble_amd.batch import PackedTextBatch
from oracle import coracle
from oracle import gosemantics as gs
from tests import key_vectors as kv
from tests.helpers import bits_from_status
from tests.test_gpu_chain_exceptions import run_bulk, run_small

pytestmark = pytest.mark.gpu

COMPACT = native.F_KEY_CACHE | native.F_KC_COMPACT
_ORACLE = {}


def oracle(name):
    """(batch, digests, statuses, bits, tags) of a layout: gosemantics'
    statuses, which the C oracle must give too (once for the module)."""
    if name not in _ORACLE:
        b, tags = kv.layouts()[name]
        want = kv.expected(b)
        h, st, bits = coracle.verify_batch(b.as_dict())
        assert np.array_equal(st, want), name
        ok = {k.tag: k.ok for k in kv.keys()}
        assert [int(x) for x in want] == [gs.REJECT if ok.get(t) else gs.REF_PANIC for t in tags], name
        _ORACLE[name] = (b, h, st, bits, tags)
    return _ORACLE[name]


# bv_api.cpp's latency rule: a bulk run of <= 4096 items from <= 256 keys (BV_LAT_TABLE_KEYS) builds K8 tables
LAT = 8
LAYOUTS = ["shift0", "shift1", "shift2", "shift3", "last"]


def check(res, h, st, bits, tags, what):
    assert np.array_equal(res.msg_hash, h), f"{what}: digests differ"
    bad = np.flatnonzero(res.status != st)
    assert bad.size == 0, f"{what}: " + ", ".join(f"{tags[i]} gpu {res.status[i]} want {st[i]}" for i in bad[:16])
    assert np.array_equal(res.accept_bits, bits), f"{what}: accept bits differ"


def verifier(monkeypatch, flags=native.F_DEFAULT, **env):
    """A Verifier created under the given environment (the knobs are read at
    bv_create)."""
    from babble_amd.verifier import Verifier

    for k, val in env.items():
        monkeypatch.setenv(k, val)
    return Verifier(device=0, flags=flags)


TABLES = dict(BV_SMALL="0", BV_TABLE_MIN_ITEMS="1", BV_K12_MIN_ITEMS="1")
GENERIC = dict(BV_SMALL="0", BV_TABLE_MIN_ITEMS="1000000", BV_LAT_TABLE_KEYS="0")


# ---------------------------------------------------------------------------
# Forged triples through tests/chaincheck
# ---------------------------------------------------------------------------
def forged():
    vecs = kv.forged_items()
    assert len(vecs) % 64 and {v.want for v in vecs} == {gs.ACCEPT, gs.REJECT, gs.REF_PANIC}
    return vecs


@pytest.mark.parametrize("path", ["K12", "K8", "generic"])
def test_forged_bulk_device_order(monkeypatch, path):
    """k_key_decode, then the key-table builders over the decoded limbs (K12,
    K8) or the per-lane generic path."""
    flags = native.F_K8 if path == "K8" else native.F_DEFAULT
    v = verifier(monkeypatch, flags, **(GENERIC if path == "generic" else TABLES))
    try:
        run_bulk(v, forged(), len(forged()), {"K12": 12, "K8": 8, "generic": 0}[path], f"forged {path}")
    finally:
        v.close()


def test_forged_bulk_host_order(monkeypatch):
    """bv_host_launch's order (k_verify_qf, then k_verify_gf in chunks) on K12
    tables."""
    v = verifier(monkeypatch, **TABLES)
    try:
        n = 2 * len(forged())  # every item twice: the chunk ends are multiples of 64 below n
        run_bulk(v, forged(), n, 12, "forged host order", ends=[64, 192])
    finally:
        v.close()


@pytest.mark.parametrize("records", [False, True], ids=["device-scalars", "host-records"])
def test_forged_small_kernel_cold(monkeypatch, records):
    """k_small without tables: the key decoded from key_bytes by wave 2
    (device-formed scalars), or from the host item record (both record sites:
    the classifying decode and the chain's)."""
    monkeypatch.delenv("BV_HOST_SCALARS", raising=False)
    v = verifier(monkeypatch)
    try:
        run_small(v, forged(), False, f"forged k_small cold records={records}", records=records)
    finally:
        v.close()


def test_forged_small_kernel_warm_kc18(monkeypatch):
    """k_small over KC18 tables.  Device-formed scalars: every item, the
    twins' keys without a table beside their canonical twins' with one.  Host
    records: the items under the good keys (a launch takes records of 16 only
    when every key has a table)."""
    monkeypatch.delenv("BV_HOST_SCALARS", raising=False)
    vecs = forged()
    good = [x for x in vecs if x.key.ok]
    v = verifier(monkeypatch, COMPACT, BV_SMALL="0")  # (the warm-up bulk call)
    try:
        v.kc_small_tables(True)
        v.register_keys(sorted({x.pub for x in vecs}))
        n_good = len({x.pub for x in good})
        t = v.timing()
        assert t["kc_builds"] == n_good == t["kc_keys"], t  # no twin gets a table
        run_bulk(v, vecs, len(vecs), 18, "forged KC18 bulk")
        assert v.timing()["kc_hits"] == n_good
        hits, n_keys = run_small(v, vecs, True, "forged k_small warm KC18")
        assert hits == n_good and n_keys == len({x.pub for x in vecs})
        hits, n_keys = run_small(v, good, True, "forged k_small warm KC18, records", records=True)
        assert hits == n_keys == n_good
    finally:
        v.close()


# ---------------------------------------------------------------------------
# Items over real bodies through the public entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_verify_small_sizes(monkeypatch, name):
    """Verifier.verify on the one-launch path: the whole layout (5..256
    items: k_small decodes from key_bytes) and slices of 1..4 items (host item
    records carry the key)."""
    monkeypatch.delenv("BV_HOST_SCALARS", raising=False)
    b, h, st, bits, tags = oracle(name)
    assert 4 < b.n_items <= 256
    v = verifier(monkeypatch)
    try:
        check(v.verify(b), h, st, bits, tags, f"{name} whole")
        t = v.timing()
        assert t["key_path"] == 0 and t["ms_h2d"] == 0, t
        lo, k = 0, 0
        while lo < b.n_items:
            hi = min(b.n_items, lo + (1, 4, 2, 3)[k % 4])
            s = shard.slice_batch(b, lo, hi)
            check(v.verify(s), h[lo:hi], st[lo:hi], bits_from_status(st[lo:hi]), tags[lo:hi], f"{name} [{lo}, {hi})")
            t = v.timing()
            assert t["key_path"] == 0 and t["ms_h2d"] == 0, (lo, hi, t)
            lo, k = hi, k + 1
    finally:
        v.close()


@pytest.mark.parametrize("path", ["K12", "K8", "generic"])
def test_verify_bulk(monkeypatch, path):
    """Verifier.verify, to_device / verify_device and verify_text with k_small
    off: k_key_decode at every alignment."""
    flags = native.F_K8 if path == "K8" else native.F_DEFAULT
    v = verifier(monkeypatch, flags, **(GENERIC if path == "generic" else TABLES))
    key_path = {"K12": 12, "K8": 8, "generic": 0}[path]
    try:
        for name in LAYOUTS:
            b, h, st, bits, tags = oracle(name)
            check(v.verify(b), h, st, bits, tags, f"{path} {name} host entry")
            t = v.timing()
            assert t["key_path"] == key_path and t["ms_h2d"] > 0, (name, t)
            d = v.to_device(b)
            v.verify_device(d)
            check(d.result(), h, st, bits, tags, f"{path} {name} device entry")
            assert v.timing()["key_path"] == key_path, name
            check(v.verify_text(text_batch(b)), h, st, bits, tags, f"{path} {name} text")
            t = v.timing()
            assert t["key_path"] == key_path and t["ms_h2d"] > 0, (name, t)
    finally:
        v.close()


def text_batch(b):
    texts = [kv.sig_text(b, i).encode()
             for i in range(b.n_items)]
    off = np.zeros(len(texts) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in texts], dtype=np.uint64)
    tb = PackedTextBatch(b.msg_bytes, b.msg_off, b.key_bytes, b.key_off, b.item_msg, b.item_key, off,
                         np.frombuffer(b"".join(texts), np.uint8).copy())
    d = tb.decoded()
    assert np.array_equal(d.r_be, b.r_be) and np.array_equal(d.s_be, b.s_be) and not d.pre.any()
    return tb


@pytest.mark.parametrize("name", LAYOUTS)
def test_verify_text_and_device_entry_small(monkeypatch, name):
    """verify_text (one launch) and the device entry (the bulk pipeline under
    the latency rule) at a latency size, defaults."""
    b, h, st, bits, tags = oracle(name)
    v = verifier(monkeypatch)
    try:
        check(v.verify_text(text_batch(b)), h, st, bits, tags, f"{name} text")
        t = v.timing()
        assert t["key_path"] == 0 and t["ms_h2d"] == 0, t
        d = v.to_device(b)
        v.verify_device(d)
        check(d.result(), h, st, bits, tags, f"{name} device entry")
        assert v.timing()["key_path"] == LAT  # no one-launch path behind the device entry
    finally:
        v.close()


def test_group_on_one_device(monkeypatch):
    """bv_group_verify_batch with one slot (bv_host_launch: the bulk
    pipeline, K8 tables by the latency rule)."""
    from babble_amd.verifier import Group

    g = Group([0])
    try:
        for name in LAYOUTS:
            b, h, st, bits, tags = oracle(name)
            check(g.verify(b), h, st, bits, tags, f"group {name}")
            assert g.timing(0)["key_path"] == LAT, name
    finally:
        g.close()


# ---------------------------------------------------------------------------
# Events, ITXs and blocks
# ---------------------------------------------------------------------------
def creator_events(shift):
    """One event per key of layout(shift) (the junk key's first), each key
    the event's creator, signed with the layout's (r, s) as text."""
    from babble_amd import events as E

    b, tags = kv.layout(shift)
    eb = E.EventBatchBuilder()
    want, digests = [], []
    for i in range(b.n_items):
        pub = b.key(i)
        sig = kv.sig_text(b, i)
        body = gs.EventBody(Transactions=[b"tx%d" % i], InternalTransactions=None, Parents=["", ""], Creator=pub,
                            Index=i, BlockSignatures=None, Timestamp=1700000000 + i)
        assert eb.add_key(pub) == i
        eb.add_event(i, i, body.Timestamp, [None, None], body.Transactions, sig)
        want.append(gs.event_status(body, sig))
        digests.append(body.Hash())
    wire = eb.pack()
    assert np.array_equal(np.asarray(wire.key_off), b.key_off)  # the layout's alignments
    ok = {k.tag: k.ok for k in kv.keys()}
    assert want == [gs.EV_REJECT if ok.get(t) else gs.EV_PANIC for t in tags]
    return wire, np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32), np.array(want, np.uint8), tags


@pytest.mark.parametrize("bulk", [False, True], ids=["small", "bulk"])
def test_events_with_the_keys_as_creators(monkeypatch, bulk):
    v = verifier(monkeypatch, **(dict(BV_SMALL="0") if bulk else {}))
    try:
        for shift in range(4):
            wire, h, st, tags = creator_events(shift)
            check(v.verify_events(wire), h, st, bits_from_status(st), tags, f"events shift {shift} bulk={bulk}")
            t = v.timing()
            assert t["key_path"] == LAT and t["ms_h2d"] > 0, (shift, t)  # (bv_verify_events has no one-launch path)
    finally:
        v.close()


def hex_forms(pub, i):
    """"0X" / "0x" and both hex cases, by turns"""
    h = pub.hex()
    return ("0X" + h.upper(), "0x" + h, "0X" + h, "0x" + h.upper())[i % 4]


def itx_specs(shift):
    """One event per key of layout(shift), validly signed by a validator,
    carrying one ITX whose PubKeyHex is the key and whose signature is the
    layout's (r, s): the ITX is REJECT (the event 4) under a good key,
    REF_PANIC (the event EV_PANIC) under a bad one."""
    from tests import itx_cases as C

    b, tags = kv.layout(shift)
    specs = []
    for i in range(b.n_items):
        sig = kv.sig_text(b, i)
        itx = C.make_itx(i % 4, netaddr="n%d" % i, moniker="m%d" % i, pubhex=hex_forms(b.key(i), i), signature=sig)
        specs.append(dict(c=i % 4, index=i, ts=1700000000 + i, txs=[b"t%d" % i], itxs=[itx]))
    return specs, tags


def check_itx(c, res, tags, what):
    st, by, ist, bits = c.expected()
    ok = {k.tag: k.ok for k in kv.keys()}
    assert [int(x) for x in ist] == [gs.REJECT if ok.get(t) else gs.REF_PANIC for t in tags], what
    assert [int(x) for x in st] == [gs.EV_ITX_INVALID if ok.get(t) else gs.EV_PANIC for t in tags], what
    assert np.array_equal(res.msg_hash, c.digests) and np.array_equal(res.itx_hash, c.itx_digests), what
    bad = np.flatnonzero(res.itx_status != ist)
    assert bad.size == 0, f"{what}: " + ", ".join(f"{tags[i]} itx gpu {res.itx_status[i]} want {ist[i]}"
                                                  for i in bad[:16])
    bad = np.flatnonzero(res.status != st)
    assert bad.size == 0, f"{what}: " + ", ".join(f"{tags[i]} event gpu {res.status[i]} want {st[i]}" for i in bad[:16])
    assert np.array_equal(res.decided_by, by) and np.array_equal(res.accept_bits, bits), what


@pytest.mark.parametrize("bulk", [False, True], ids=["small", "bulk"])
def test_events_with_the_keys_as_itx_pubkeyhex(monkeypatch, bulk):
    """bv_verify_events_itx and bv_verify_events_fields: the key bytes come
    out of the device's hex decoder."""
    from tests import fields_cases as F
    from tests import itx_cases as C

    v = verifier(monkeypatch, **(dict(BV_SMALL="0") if bulk else {}))
    try:
        for shift in range(4):
            specs, tags = itx_specs(shift)
            c = C.ItxCase(specs)
            assert c.n + c.packed.n_itx <= 256
            check_itx(c, v.verify_events_itx(c.packed), tags, f"events_itx shift {shift} bulk={bulk}")
            t = v.timing()
            assert t["key_path"] == (LAT if bulk else 0) and (t["ms_h2d"] > 0) == bulk, (shift, t)
            for e, s in enumerate(specs):
                s["bsigs"] = [F.block_sig(e % 4, e, e)] if e % 3 == 0 else None
            f = F.FieldsCase(specs)
            check_itx(f, v.verify_events_fields(f.packed), tags, f"events_fields shift {shift} bulk={bulk}")
            t = v.timing()
            assert t["key_path"] == (LAT if bulk else 0) and (t["ms_h2d"] > 0) == bulk, (shift, t)
    finally:
        v.close()


@pytest.mark.parametrize("bulk", [False, True], ids=["small", "bulk"])
def test_blocks_with_the_keys_as_validators(monkeypatch, bulk):
    """bv_verify_blocks: two blocks, every key of the layout a validator of
    both."""
    from tests import block_cases as BC

    v = verifier(monkeypatch, **(dict(BV_SMALL="0") if bulk else {}))
    try:
        for shift in range(4):
            b, tags = kv.layout(shift)
            keys = [b.key(k) for k in range(b.n_keys)]
            bodies = [gs.BlockBody(1 + j, 2, 1700000000, b"s", b"f", b"p", [b"tx%d" % j], None, None) for j in range(2)]
            items = [(j, k, kv.sig_text(b, k))
                     for j in range(2) for k in range(len(keys))]
            c = BC.BlockCase(bodies, items, 0, extra_keys=keys)
            assert np.array_equal(np.asarray(c.fields.key_off), b.key_off)
            h, st, bits = c.oracle()
            ok = {k.tag: k.ok for k in kv.keys()}
            assert [int(x) for x in st] == 2 * [gs.REJECT if ok.get(t) else gs.REF_PANIC for t in tags]
            res = v.verify_blocks(c.fields)
            check(res, c.digests, st, bits, 2 * tags, f"blocks shift {shift} bulk={bulk}")
            assert not res.valid_count.any()
            t = v.timing()
            assert t["key_path"] == (LAT if bulk else 0) and (t["ms_h2d"] > 0) == bulk, (shift, t)
    finally:
        v.close()


# ---------------------------------------------------------------------------
# Key cache
# ---------------------------------------------------------------------------
def n_good(b):
    return len({b.key(k) for k in range(b.n_keys) if gs.Unmarshal(b.key(k)) is not None})


@pytest.mark.parametrize("small_tables", [False, True], ids=["small-tables-off", "small-tables-on"])
def test_kc18_registered(monkeypatch, small_tables):
    """Every vector key registered on a KC18 context: a table per good key,
    none for a twin; then mixed batches three times each (the bad-key memo is
    filled by the registration and hit by every batch), on the one-launch
    path, in slices that carry host records, and on the bulk path."""
    monkeypatch.delenv("BV_HOST_SCALARS", raising=False)
    b, h, st, bits, tags = oracle("shift1")
    good = n_good(b)
    assert good == sum(k.ok for k in kv.keys())
    v = verifier(monkeypatch, COMPACT)
    w = verifier(monkeypatch, COMPACT, BV_SMALL="0")
    try:
        for x in (v, w):
            x.register_keys([k.pub for k in kv.keys()])
            t = x.timing()
            assert t["kc_builds"] == good == t["kc_keys"], t
            x.kc_small_tables(small_tables)
        for rep in range(3):
            for name in ("shift1", "last"):
                b, h, st, bits, tags = oracle(name)
                check(v.verify(b), h, st, bits, tags, f"KC18 small {name} #{rep}")
                t = v.timing()
                want = (18, good, 0, 0) if small_tables else (0, 0, 0, 0)
                assert (t["key_path"], t["kc_hits"], t["kc_builds"], t["ms_h2d"]) == want, (name, rep, t)
                assert t["kc_keys"] == good
                check(w.verify(b), h, st, bits, tags, f"KC18 bulk {name} #{rep}")
                t = w.timing()
                got = (t["key_path"], t["kc_hits"], t["kc_builds"], t["kc_keys"])
                assert got == (18, good, 0, good), (name, rep, t)
        b, h, st, bits, tags = oracle("shift1")
        lo, k = 0, 0
        while lo < b.n_items:  # records: a twin beside its canonical twin, whose table the record names
            hi = min(b.n_items, lo + (4, 16, 3, 2, 9)[k % 5])
            s = shard.slice_batch(b, lo, hi)
            check(v.verify(s), h[lo:hi], st[lo:hi], bits_from_status(st[lo:hi]), tags[lo:hi], f"KC18 [{lo}, {hi})")
            t = v.timing()
            assert t["key_path"] == (18 if small_tables else 0), (lo, hi, t)
            assert t["kc_builds"] == 0 and t["ms_h2d"] == 0, (lo, hi, t)
            lo, k = hi, k + 1
    finally:
        v.close()
        w.close()


def kc22_batch():
    """two good keys (a small x, a small y), their two twins and the junk key"""
    tags = ["x/1/y0", "x+p/1/y0", f"y/{kv.small_y_values()[0][-1]}/r1/lo", f"y+p/{kv.small_y_values()[0][-1]}/r1"]
    order = [i for i, k in enumerate(kv.keys()) if k.tag in tags]
    assert len(order) == 4
    b, t = kv.layout(3, order=order)
    want = kv.expected(b)
    h, st, bits = coracle.verify_batch(b.as_dict())
    assert np.array_equal(st, want) and sorted(st.tolist()) == [0, 0, 3, 3, 3]
    return b, h, st, bits, t


@pytest.mark.parametrize("bulk", [False, True], ids=["small", "bulk"])
def test_kc22_registered(monkeypatch, bulk):
    b, h, st, bits, tags = kc22_batch()
    v = verifier(monkeypatch, native.F_KEY_CACHE, **(dict(BV_SMALL="0") if bulk else {}))
    try:
        v.register_keys([b.key(k) for k in range(1, b.n_keys)])
        t = v.timing()
        assert t["kc_builds"] == 2 == t["kc_keys"], t
        for rep in range(3):
            check(v.verify(b), h, st, bits, tags, f"KC22 bulk={bulk} #{rep}")
            t = v.timing()
            assert (t["key_path"], t["kc_hits"], t["kc_builds"], t["kc_keys"]) == (22, 2, 0, 2), (rep, t)
            assert (t["ms_h2d"] > 0) == bulk, t
    finally:
        v.close()


def test_admission_never_builds_a_table_for_a_twin(monkeypatch):
    """An unregistered KC18 context that admits a key at first sight: the
    first batch builds a table per good key, the twins (seen three times in
    a row) never get one, and no status ever changes."""
    b, h, st, bits, tags = oracle("shift2")
    good = n_good(b)
    v = verifier(monkeypatch, COMPACT, BV_SMALL="0", BV_KC_ADMIT="1")
    try:
        for rep in range(3):
            check(v.verify(b), h, st, bits, tags, f"admission #{rep}")
            t = v.timing()
            want = (18, 0, good, good) if rep == 0 else (18, good, 0, good)
            assert (t["key_path"], t["kc_hits"], t["kc_builds"], t["kc_keys"]) == want, (rep, t)
    finally:
        v.close()
