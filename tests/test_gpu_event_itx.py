"""bv_verify_events_itx on the device: Event.Verify with the
InternalTransactions from fields, one call (k_itx_body_hash,
k_ev_body_hash_itx, k_ev_compose; babble_amd/csrc/itxjson.h).

Judge: oracle/gosemantics.py (EventBody.Marshal, InternalTransactionBody
.Marshal, itx_status, event_status, event_verify_error) and hashlib for the
digests.  Every event and every ITX of every batch is compared.  Workloads:
tests/itx_cases.py."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from babble_amd import events as E
from babble_amd import hashgraph as H
from babble_amd import native
from babble_amd.verifier import Verifier
from oracle import gosemantics as G
from tests import itx_cases as C

pytestmark = pytest.mark.gpu

_cases = {}


def cached(name, make):
    if name not in _cases:
        _cases[name] = make()
    return _cases[name]


@pytest.fixture(scope="module")
def v0():
    v = Verifier(0)
    yield v
    v.close()


def check(c: C.ItxCase, res, what=""):
    st, by, ist, bits = c.expected()
    assert np.array_equal(res.msg_hash, c.digests), (what, np.flatnonzero((res.msg_hash != c.digests).any(axis=1))[:8])
    assert np.array_equal(res.itx_hash, c.itx_digests), (what,
                                                         np.flatnonzero((res.itx_hash != c.itx_digests).any(axis=1))[:8])
    assert np.array_equal(res.itx_status, ist), (what, np.flatnonzero(res.itx_status != ist)[:8])
    assert np.array_equal(res.status, st), (what, np.flatnonzero(res.status != st)[:8], res.status[:16], st[:16])
    assert np.array_equal(res.decided_by, by), (what, np.flatnonzero(res.decided_by != by)[:8])
    assert np.array_equal(res.accept_bits, bits), what


@pytest.fixture(scope="module")
def vbulk():
    """A context whose host entries never take the one-launch small path
    (BV_SMALL=0, read at creation): every batch runs the bulk pipeline's
    kernels, whatever its size."""
    old = os.environ.get("BV_SMALL")
    os.environ["BV_SMALL"] = "0"
    try:
        v = Verifier(0)
    finally:
        if old is None:
            del os.environ["BV_SMALL"]
        else:
            os.environ["BV_SMALL"] = old
    yield v
    v.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_lane_and_word_boundaries(vbulk, n):
    """Bulk batches whose ITX lists cycle nil / [] / 1 / 2 / 3, valid
    signatures mixed with corrupted ones (the specs of n events are the first
    n of the 130-event batch's)."""
    c = cached(("cycle", n), lambda: C.ItxCase(C.cycle_specs(130)[:n]))
    st = c.expected()[0]
    if n >= 63:
        assert {0, 1, 4} <= set(st.tolist())
    check(c, vbulk.verify_events_itx(c.packed), n)
    if c.packed.n_itx:
        assert vbulk.timing()["ms_h2d"] > 0  # staged: the bulk pipeline


@pytest.mark.parametrize("n", [3, 63, 65])
def test_small_batches_take_the_one_launch_path(n):
    """A key-cache context with the creators registered and a batch small
    enough for the one-launch path: nothing is staged (ms_h2d == 0), the
    results are the oracle's."""
    c = cached(("cycle", n), lambda: C.ItxCase(C.cycle_specs(130)[:n]))
    assert 0 < c.packed.n_itx and n + c.packed.n_itx <= 256
    v = Verifier(0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys([pub for _, pub in C.validators(4)])
        check(c, v.verify_events_itx(c.packed), n)
        t = v.timing()
        assert t["ms_h2d"] == 0, t
    finally:
        v.close()


def fold_specs():
    v = C.validators(4)
    good = lambda k, **kw: C.make_itx(k % 4, netaddr="a%d" % k, **kw)  # noqa: E731
    off_curve = "0X04" + "11" * 64
    long_key = "0X04" + "22" * 69  # 70 bytes
    cases = [
        dict(itxs=[good(0), good(1, good=False), good(2, pubhex="0")]),               # 4, decided by 1
        dict(itxs=[good(0), good(1)], good=False),                                    # REJECT, SELF
        dict(itxs=[good(0), good(1, signature="onepart")]),                           # REJECT_ERR
        dict(itxs=[good(0, pubhex="", signature="onepart")]),                         # REF_PANIC (precedence)
        dict(itxs=[good(0, pubhex="0", signature="one|two|three")]),                  # REF_PANIC (precedence)
        dict(itxs=[good(1, pubhex="0X")]),                                            # empty key, valid text
        dict(itxs=[good(1, pubhex="0X", signature="onepart")]),                       # empty key: REJECT_ERR first
        dict(itxs=[good(2, pubhex=C.pub_hex(v[2][1]) + "A")]),                        # odd length: the key decodes
        dict(itxs=[good(2, pubhex=C.pub_hex(v[2][1])[:40] + "G" + C.pub_hex(v[2][1])[41:])]),  # partial decode
        dict(itxs=[good(3, pubhex=long_key)]),
        dict(itxs=[good(3, pubhex=off_curve)]),
        dict(c=0, itxs=[good(0)]),                                                    # the creator's key is the ITX's
        dict(itxs=[good(0), good(1), good(2)]),
        dict(itxs=[]),
        dict(itxs=None),
    ]
    specs = []
    for e in range(64):
        s = dict(cases[e % len(cases)]) if e < 2 * len(cases) else dict(itxs=None)
        s.setdefault("c", e % 4)
        s.update(index=e, ts=1700000000 + e, txs=[b"tx%d" % e])
        if e >= len(cases) and e < 2 * len(cases):
            s["good"] = not s.get("good", True)  # the same ITX lists under the other event outcome
        specs.append(s)
    return specs


@pytest.mark.parametrize("route", ["default", "bulk"])
def test_fold_table(v0, vbulk, route):
    v0 = vbulk if route == "bulk" else v0
    c = cached("fold", lambda: C.ItxCase(fold_specs()))
    assert c.n == 64
    st, by, ist, _ = c.expected()
    assert (st[0], by[0]) == (4, 1) and (st[1], by[1]) == (0, C.EV_SELF) and (st[2], by[2]) == (2, 1)
    assert st[3] == 3 and st[4] == 3 and st[5] == 3 and st[6] == 2 and st[11] == 1
    assert set(st.tolist()) == {0, 1, 2, 3, 4}
    res = v0.verify_events_itx(c.packed)
    check(c, res, "fold")
    # the mirror: Go's (ok, err) / panic for every event, the error texts included
    evs = [H.Event(Body=H.EventBody(
        Transactions=b.Transactions, Parents=b.Parents, Creator=b.Creator, Index=b.Index, Timestamp=b.Timestamp,
        InternalTransactions=None if b.InternalTransactions is None else [
            H.InternalTransaction(H.InternalTransactionBody(t.Body.Type, H.Peer(t.Body.Peer.NetAddr, t.Body.Peer.PubKeyHex,
                                                                                t.Body.Peer.Moniker)), t.Signature)
            for t in b.InternalTransactions]), Signature=s) for b, s in zip(c.bodies, c.signatures)]
    outs = H.verify_events(evs, v0, fields=True)
    for e, (o, b, s) in enumerate(zip(outs, c.bodies, c.signatures)):
        assert o.ok == (st[e] == 1) and o.panic == (st[e] == 3), e
        if st[e] == 2:
            assert o.err == G.event_verify_error(b, s), e
        if st[e] == 4:
            assert o.err == "invalid signature on internal transaction", e
        assert evs[e]._hash == c.digests[e].tobytes()
    assert outs[2].err == "wrong number of values in signature: got 1, want 2"
    assert outs[3].err == "slice bounds out of range"


def digest_case(monikers):
    return C.ItxCase([dict(c=e % 4, index=e, itxs=[G.InternalTransaction(
        G.InternalTransactionBody(1, G.Peer("", "", m)), "")], signature="1|2") for e, m in enumerate(monikers)])


def test_escapes_on_the_device(v0):
    """Every single byte and every lead x trail pair as the Moniker of one ITX
    per event: the ITX and event digests."""
    c = cached("escapes", lambda: digest_case([bytes([b]) for b in range(256)] + C.pair_strings()))
    assert c.n == 328
    res = v0.verify_events_itx(c.packed)
    assert np.array_equal(res.itx_hash, c.itx_digests), np.flatnonzero((res.itx_hash != c.itx_digests).any(axis=1))[:8]
    assert np.array_equal(res.msg_hash, c.digests), np.flatnonzero((res.msg_hash != c.digests).any(axis=1))[:8]


def test_padding_residues(v0):
    """ITX bodies of every length mod 64 (the 61-byte minimal body plus a
    Moniker of 0..130 bytes: the 55/56 and 63/64 padding edges twice)."""
    c = cached("residues", lambda: digest_case([b"m" * k for k in range(131)]))
    assert len(c.itx_raw[0]) == 61 and {len(r) % 64 for r in c.itx_raw} == set(range(64))
    res = v0.verify_events_itx(c.packed)
    assert np.array_equal(res.itx_hash, c.itx_digests)
    assert np.array_equal(res.msg_hash, c.digests)


def dag_specs():
    specs = []
    for e in range(40):
        c = e % 4
        par = [("event", e - 4) if e >= 4 else None, ("event", e - 1) if e >= 1 else None]
        itxs = None
        if e % 3 == 1:
            itxs = [C.make_itx((e + j) % 4, netaddr="d%d" % e, moniker="<%d&%d>" % (e, j), good=(e + j) % 5 != 0)
                    for j in range(1 + e % 2)]
        specs.append(dict(c=c, index=e // 4, ts=1650000000 + e, parents=par, txs=[b"t" * (e % 5)], itxs=itxs,
                          good=e % 6 != 5))
    return specs


@pytest.mark.parametrize("route", ["default", "bulk"])
def test_dag_batch_and_the_two_call_path(v0, vbulk, route):
    v0 = vbulk if route == "bulk" else v0
    """40 events of 4 creators in 40 levels, ITXs on events with in-batch
    parents: the oracle, and today's sequence (bv_verify_events over the ITX
    fragments, the ITX items in a second call, the fold on the host)."""
    c = cached("dag", lambda: C.ItxCase(dag_specs()))
    assert c.packed.n_itx > 10 and (c.packed.events.parent_kind == E.PARENT_EVENT).sum() > 60
    res = v0.verify_events_itx(c.packed)
    check(c, res, "dag")
    frag = E.EventBatchBuilder()
    for k in range(4):
        frag.add_key(C.validators(4)[k][1])
    for s, b, sig in zip(dag_specs(), c.bodies, c.signatures):
        frag.add_event(s["c"], b.Index, b.Timestamp, s["parents"], b.Transactions, sig,
                       itx_json=b"" if b.InternalTransactions is None else G.json_list(b.InternalTransactions,
                                                                                      lambda t: t.json()))
    two = v0.verify_events(frag.pack())
    assert np.array_equal(two.msg_hash, res.msg_hash)
    flat = [H.InternalTransaction(H.InternalTransactionBody(t.Body.Type, H.Peer(
        t.Body.Peer.NetAddr, t.Body.Peer.PubKeyHex, t.Body.Peer.Moniker)), t.Signature) for t in c.itxs]
    outs = H.verify_itxs(flat, v0)
    k = 0
    for e, b in enumerate(c.bodies):
        m = len(b.InternalTransactions or [])
        own = [1 if o.ok else 3 if o.panic else 2 if o.err else 0 for o in outs[k:k + m]]
        assert own == res.itx_status[k:k + m].tolist(), e
        o = H.compose_event_outcome(own, int(two.status[e]), [t.Signature for t in flat[k:k + m]], c.signatures[e])
        folded = 1 if o.ok else 3 if o.panic else 4 if o.err == "invalid signature on internal transaction" else \
            2 if o.err else 0
        assert folded == res.status[e], e
        k += m


def test_no_itx_equals_verify_events(v0):
    """n_itx == 0: status, hash and bits are bv_verify_events' over the same
    events with nil / [] fragments."""
    specs = [dict(s, itxs=None if e % 2 else []) for e, s in enumerate(C.cycle_specs(70))]
    c = cached("none", lambda: C.ItxCase(specs))
    assert c.packed.n_itx == 0
    res = v0.verify_events_itx(c.packed)
    check(c, res, "no itx")
    frag = E.EventBatchBuilder()
    for k in range(4):
        frag.add_key(C.validators(4)[k][1])
    for s, b, sig in zip(specs, c.bodies, c.signatures):
        frag.add_event(s["c"], b.Index, b.Timestamp, s["parents"], b.Transactions, sig,
                       itx_json=b"" if b.InternalTransactions is None else b"[]")
    ref = v0.verify_events(frag.pack())
    assert np.array_equal(ref.msg_hash, res.msg_hash) and np.array_equal(ref.status, res.status)
    assert np.array_equal(ref.accept_bits, res.accept_bits)
    assert (res.decided_by == C.EV_SELF).all()


def test_argument_errors_then_a_valid_call(v0):
    c = cached(("cycle", 65), lambda: C.ItxCase(C.cycle_specs(130)[:65]))
    p = c.packed
    m = p.n_itx

    def bad(xb=None, patch=None):
        keep = []
        cb = (xb or p).c_struct(keep)
        if patch:
            patch(cb)
        h = np.zeros((p.n_events, 32), np.uint8)
        res = native.BvResult(h.ctypes.data, None, None)
        rc = v0._L.bv_verify_events_itx(v0._ctx, ctypes.byref(cb), ctypes.byref(res), None)
        assert rc == native.BV_E_ARGS, rc
        assert v0._L.bv_last_error(v0._ctx)

    def rep(**kw):
        return dataclasses.replace(p, **kw)

    def arr(a, i, v):
        a = np.array(a, copy=True)
        a[i] = v
        return a

    one = np.ones(4, np.uint64)
    bad(patch=lambda cb: setattr(cb.events, "itx_off", one.ctypes.data))
    bad(patch=lambda cb: setattr(cb.events, "itx_json", one.ctypes.data))
    bad(patch=lambda cb: setattr(cb.events, "sig_text", None))
    bad(patch=lambda cb: setattr(cb, "itx_start", None))
    bad(rep(itx_start=arr(p.itx_start, 0, 1)))
    bad(rep(itx_start=arr(p.itx_start, 3, int(p.itx_start[-1]) + 1)))
    huge = np.zeros_like(p.itx_start)
    huge[-1] = (1 << 32) + 1  # n_events + n_itx > 2^32 (nothing past itx_start is read)
    bad(rep(itx_start=huge))
    bad(patch=lambda cb: setattr(cb, "itx_str_off", None))
    bad(rep(itx_str_off=arr(p.itx_str_off, 0, 1)))
    bad(rep(itx_str_off=arr(p.itx_str_off, 2, int(p.itx_str_off[-1]) + 1)))
    bad(patch=lambda cb: setattr(cb, "itx_str", None))
    bad(patch=lambda cb: setattr(cb, "itx_type", None))
    # what bv_verify_events rejects: a creator out of range, an in-batch parent that is not earlier
    bad(rep(events=dataclasses.replace(p.events, creator=arr(p.events.creator, 5, 99))))
    pk, pr = arr(p.events.parent_kind, (0, 0), E.PARENT_EVENT), arr(p.events.parent_ref, (0, 0), 0)
    bad(rep(events=dataclasses.replace(p.events, parent_kind=pk, parent_ref=pr)))
    assert m > 0
    check(c, v0.verify_events_itx(p), "after the errors")
