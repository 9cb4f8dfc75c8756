"""InternalTransactions from fields on the CPU (babble_amd/csrc/itxjson.h,
bv_event_itx.cpp's host helpers, the Python mirror).

Judge: oracle/gosemantics.py (json_string, InternalTransactionBody.Marshal,
EventBody.Marshal, itx_status, event_status, event_verify_error) and hashlib.
The serialiser's public form (bv_itx_bodies, bv_event_itx_bodies) is compared
byte for byte; the device's streaming sink runs on the host (tests/emu_itx);
an ASan + UBSan driver with its own main fuzzes the emit and length functions.
The GPU half is tests/test_gpu_event_itx.py.  Workloads: tests/itx_cases.py."""
import ctypes
import dataclasses
import hashlib
import subprocess

import numpy as np
import pytest

from babble_amd import events as E
from babble_amd import hashgraph as H
from babble_amd import native, sync
from oracle import gosemantics as G
from tests import itx_cases as C
from tests.emu_itx import emu_itx

_cases = {}


def cached(name, make):
    if name not in _cases:
        _cases[name] = make()
    return _cases[name]


def grid_case(pos):
    return cached(("grid", pos), lambda: C.ItxCase(
        [dict(c=e % 4, index=e, itxs=[C.string_itx(s, pos)], signature="1|2") for e, s in enumerate(C.string_grid())]))


def test_gojson_string_equals_the_oracle_over_the_grid():
    for s in C.string_grid():
        out, n = emu_itx.string(s)
        assert out == G.json_string(s), s
        assert n == len(out), s


@pytest.mark.parametrize("pos", [0, 1, 2, 3])
def test_string_grid_in_every_position(pos):
    """bv_itx_bodies and bv_event_itx_bodies equal the oracle byte for byte
    with every grid string as NetAddr / PubKeyHex / Moniker / Signature, and
    every *_len equals the emitted length."""
    c = grid_case(pos)
    assert c.packed.n_itx == 2345
    assert c.packed.itx_bodies() == c.itx_raw
    assert c.packed.event_bodies() == c.raw
    for kind, want in ((0, [len(r) for r in c.itx_raw]), (1, [len(t.json()) for t in c.itxs]),
                       (2, [len(r) for r in c.raw])):
        lens, emitted = emu_itx.lens(c.packed, kind)
        assert lens.tolist() == want and emitted.tolist() == want, kind


def body_specs():
    """nil / [] / 1 / 3 ITXs crossed with the Transactions options (nil, [],
    a nil transaction, empty, several) and the parent options (none, hash,
    in-batch) of the events tests."""
    specs = []
    tx_opts = [None, [], [None], [b""], [b"a", None, b"\x00" * 33], [bytes(range(64))]]
    itx_opts = [lambda e: None, lambda e: [], lambda e: [C.make_itx(e % 4, moniker="<%d>" % e)],
                lambda e: [C.make_itx((e + j) % 4, typ=j, netaddr="h\"%d\\%d" % (e, j)) for j in range(3)]]
    e = 0
    for txs in tx_opts:
        for mk in itx_opts:
            for par in range(5):
                h = hashlib.sha256(b"p%d" % e).digest()
                parents = [[None, None], [("hash", h), None], [None, ("hash", h)],
                           [("event", max(e - 1, 0)), ("hash", h)], [("event", max(e - 2, 0)), ("event", max(e - 1, 0))]][par]
                if e == 0:
                    parents = [None, None]
                specs.append(dict(c=e % 4, index=e - 3, ts=1600000000 - e, parents=parents, txs=txs, itxs=mk(e)))
                e += 1
    return specs


def test_event_bodies_and_parent_positions():
    c = cached("bodies", lambda: C.ItxCase(body_specs()))
    p = c.packed
    assert c.n == 120 and (p.events.parent_kind == E.PARENT_EVENT).any()
    got = p.event_bodies()
    zero = b"0" * 64
    for e, (g, body) in enumerate(zip(got, c.bodies)):
        # the oracle's body with every in-batch parent's hex as the placeholder
        ps = [("0X" + zero.decode()) if p.events.parent_kind[e, k] == E.PARENT_EVENT else s
              for k, s in enumerate(body.Parents)]
        want = dataclasses.replace(body, Parents=ps).Marshal()
        assert g == want, e
        pp = emu_itx.ppos(p, e)
        for k in range(2):
            if p.events.parent_kind[e, k] == E.PARENT_EVENT:
                assert g[pp[k] - 3:pp[k]] == b'"0X' and g[pp[k]:pp[k] + 64] == zero, (e, k)
                assert pp[k] > g.index(b',"Parents":['), (e, k)  # after the ITX text
            else:
                assert pp[k] == 0xFFFFFFFF, (e, k)
    assert p.itx_bodies() == c.itx_raw
    lens, emitted = emu_itx.lens(p, 2)
    assert lens.tolist() == emitted.tolist() == [len(g) for g in got]


def residue_case():
    return C.ItxCase([dict(c=e % 4, index=e, itxs=[G.InternalTransaction(
        G.InternalTransactionBody(1, G.Peer("", "", b"m" * e)), "")], signature="1|2") for e in range(131)])


def test_streaming_sink_at_every_padding_residue():
    """The EvjSha path built for the host equals hashlib for ITX bodies of
    every length mod 64 (the 61-byte minimal body, Moniker of 0..130 bytes)
    and for the event bodies that carry them."""
    c = cached("residues", residue_case)
    assert len(c.itx_raw[0]) == 61 and {len(r) % 64 for r in c.itx_raw} == set(range(64))
    assert {55, 56, 63, 0} <= {len(r) % 64 for r in c.itx_raw}
    assert np.array_equal(emu_itx.itx_body_hash(c.packed), c.itx_digests)
    assert np.array_equal(emu_itx.ev_body_hash(c.packed), c.digests)
    assert len({len(r) % 64 for r in c.raw}) == 64


def test_streaming_sink_over_the_grid_and_the_bodies():
    for c in (grid_case(2), cached("bodies", lambda: C.ItxCase(body_specs()))):
        assert np.array_equal(emu_itx.itx_body_hash(c.packed), c.itx_digests)
    c = grid_case(3)
    assert np.array_equal(emu_itx.ev_body_hash(c.packed), c.digests)


def test_sanitizer_fuzz_driver():
    exe = emu_itx.fuzz_exe()
    for seed in (1, 2, 3):
        r = subprocess.run([exe, str(seed), "150"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), (seed, r.stdout[-400:], r.stderr[-2000:])


def test_host_helper_argument_checks():
    L = native.lib()
    c = cached("bodies", lambda: C.ItxCase(body_specs()))
    p = c.packed
    off_i = np.zeros(p.n_itx + 1, np.uint64)
    off_e = np.zeros(p.n_events + 1, np.uint64)
    out = np.zeros(1 << 20, np.uint8)

    def call(xb, patch=None):
        keep = []
        cb = xb.c_struct(keep)
        if patch:
            patch(cb)
        return (L.bv_itx_body_lens(ctypes.byref(cb), off_i.ctypes.data),
                L.bv_event_itx_body_lens(ctypes.byref(cb), off_e.ctypes.data))

    def arr(a, i, v):
        a = np.array(a, copy=True)
        a[i] = v
        return a

    assert call(p) == (native.BV_OK, native.BV_OK)
    assert L.bv_itx_body_lens(None, off_i.ctypes.data) == native.BV_E_ARGS
    keep = []
    cb = p.c_struct(keep)
    assert L.bv_itx_body_lens(ctypes.byref(cb), None) == native.BV_E_ARGS
    assert L.bv_event_itx_body_lens(ctypes.byref(cb), None) == native.BV_E_ARGS
    both = (native.BV_E_ARGS, native.BV_E_ARGS)
    one = np.ones(4, np.uint64)
    assert call(p, lambda cb: setattr(cb.events, "itx_off", one.ctypes.data)) == both
    assert call(p, lambda cb: setattr(cb, "itx_start", None)) == both
    assert call(dataclasses.replace(p, itx_start=arr(p.itx_start, 0, 1))) == both
    assert call(dataclasses.replace(p, itx_start=arr(p.itx_start, 4, 10**6))) == both
    assert call(p, lambda cb: setattr(cb, "itx_str_off", None)) == both
    assert call(dataclasses.replace(p, itx_str_off=arr(p.itx_str_off, 0, 1))) == both
    assert call(dataclasses.replace(p, itx_str_off=arr(p.itx_str_off, 1, 10**9))) == both
    assert call(p, lambda cb: setattr(cb, "itx_str", None)) == both
    assert call(p, lambda cb: setattr(cb, "itx_type", None)) == both
    huge = np.zeros_like(p.itx_start)
    huge[-1] = (1 << 32) + 1
    assert call(dataclasses.replace(p, itx_start=huge)) == both
    # the event fields are checked only by the event-body helpers
    bad_creator = dataclasses.replace(p, events=dataclasses.replace(p.events, creator=arr(p.events.creator, 2, 77)))
    assert call(bad_creator) == (native.BV_OK, native.BV_E_ARGS)
    # bodies: offsets too short for a body, a NULL output
    assert call(p) == (native.BV_OK, native.BV_OK)
    keep = []
    cb = p.c_struct(keep)
    assert L.bv_itx_bodies(ctypes.byref(cb), off_i.ctypes.data, out.ctypes.data) == native.BV_OK
    assert L.bv_itx_bodies(ctypes.byref(cb), off_i.ctypes.data, None) == native.BV_E_ARGS
    assert L.bv_event_itx_bodies(ctypes.byref(cb), off_e.ctypes.data, None) == native.BV_E_ARGS
    short_i, short_e = off_i.copy(), off_e.copy()
    short_i[1:] -= 1
    short_e[1:] -= 1
    assert L.bv_itx_bodies(ctypes.byref(cb), short_i.ctypes.data, out.ctypes.data) == native.BV_E_ARGS
    assert L.bv_event_itx_bodies(ctypes.byref(cb), short_e.ctypes.data, out.ctypes.data) == native.BV_E_ARGS


# ----------------------------------------------------------------------------
# the Python mirror over a stub verifier that answers from the oracle
# ----------------------------------------------------------------------------
class OracleVerifier:
    """verify_events_itx answered by the oracle from the packed fields alone
    (bodies through the library's host serialiser; no device)."""

    def __init__(self):
        self.calls = 0

    def verify_events_itx(self, xb):
        from babble_amd.verifier import EventItxVerifyResult

        self.calls += 1
        n, m = xb.n_events, xb.n_itx
        ev = xb.events
        assert not (ev.parent_kind == E.PARENT_EVENT).any()  # (placeholders would not hash to Event.Hash)
        bodies, ibodies = xb.event_bodies(), xb.itx_bodies()
        so, raw = xb.itx_str_off, xb.itx_str.tobytes()
        strs = [raw[int(so[k]):int(so[k + 1])] for k in range(4 * m)]
        sigs = [ev.sig_text.tobytes()[int(ev.sig_off[e]):int(ev.sig_off[e + 1])] for e in range(n)]
        keys = [ev.key_bytes.tobytes()[int(ev.key_off[k]):int(ev.key_off[k + 1])] for k in range(len(ev.key_off) - 1)]
        ist = []
        for i in range(m):
            t = G.InternalTransaction(G.InternalTransactionBody(int(xb.itx_type[i]), G.Peer(*strs[4 * i:4 * i + 3])),
                                      strs[4 * i + 3])
            assert t.Body.Marshal() == ibodies[i]
            ist.append(G.itx_status(t))
        st, by = [], []
        for e in range(n):
            own = ist[int(xb.itx_start[e]):int(xb.itx_start[e + 1])]
            first = next((j for j, c in enumerate(own) if c != G.ACCEPT), None)
            if first is None:
                by.append(E.EV_SELF)
                st.append(G.item_status_from_sigstr(keys[int(ev.creator[e])], hashlib.sha256(bodies[e]).digest(), sigs[e]))
            else:
                by.append(first)
                st.append(4 if own[first] == G.REJECT else own[first])
        h = np.frombuffer(b"".join(hashlib.sha256(b).digest() for b in bodies), np.uint8).reshape(n, 32)
        ih = np.frombuffer(b"".join(hashlib.sha256(b).digest() for b in ibodies), np.uint8).reshape(m, 32)
        st = np.array(st, np.uint8)
        return EventItxVerifyResult(h, st, np.zeros((n + 63) // 64, np.uint64), ih, np.array(ist, np.uint8),
                                    np.array(by, np.uint32))


def mirror_itx(t):
    return H.InternalTransaction(H.InternalTransactionBody(t.Body.Type, H.Peer(t.Body.Peer.NetAddr, t.Body.Peer.PubKeyHex,
                                                                             t.Body.Peer.Moniker)), t.Signature)


def mirror_specs():
    good = lambda k, **kw: C.make_itx(k % 4, netaddr="a%d" % k, **kw)  # noqa: E731
    lists = [None, [], [good(0)], [good(0), good(1, good=False), good(2, pubhex="0")],
             [good(0), good(1, signature="one|two|three")], [good(0, pubhex="", signature="onepart")],
             [good(1, pubhex="0X")], [good(0), good(1)]]
    h = hashlib.sha256(b"known").digest()
    specs = []
    for e in range(2 * len(lists)):
        specs.append(dict(c=e % 4, index=e, ts=5 + e, parents=[("hash", h), None], txs=[b"x"], itxs=lists[e % len(lists)],
                          good=e < len(lists)))
    specs.append(dict(c=0, index=99, itxs=[good(3)], signature="nobar"))
    return specs


def test_mirror_verify_events_fields_over_the_oracle_stub():
    c = cached("mirror", lambda: C.ItxCase(mirror_specs()))
    evs = [H.Event(Body=H.EventBody(
        Transactions=b.Transactions, Parents=b.Parents, Creator=b.Creator, Index=b.Index, Timestamp=b.Timestamp,
        InternalTransactions=None if b.InternalTransactions is None else [mirror_itx(t) for t in b.InternalTransactions]),
        Signature=s) for b, s in zip(c.bodies, c.signatures)]
    stub = OracleVerifier()
    outs = H.verify_events(evs, stub, fields=True)
    assert stub.calls == 1
    st = c.expected()[0]
    assert set(st.tolist()) == {0, 1, 2, 3, 4}
    for e, (o, b, s) in enumerate(zip(outs, c.bodies, c.signatures)):
        assert o.ok == (st[e] == 1) and o.panic == (st[e] == 3), e
        if st[e] == 2:
            assert o.err == G.event_verify_error(b, s), e
        elif st[e] == 4:
            assert o.err == "invalid signature on internal transaction", e
        elif st[e] in (0, 1):
            assert o.err is None, e
        assert evs[e]._hash == c.digests[e].tobytes(), e
    assert outs[4].err == "wrong number of values in signature: got 3, want 2"
    assert outs[5].err == "slice bounds out of range" and outs[5].panic
    assert outs[-1].err == "wrong number of values in signature: got 1, want 2"
    with pytest.raises(ValueError):
        H.verify_events([H.Event(Body=H.EventBody(Parents=["", "0Xzz"], Creator=b"k"), Signature="1|2")], stub,
                        fields=True)


def test_sync_keyword_drops_the_second_call():
    """sync_verify_device(fields=True): one verify_events_itx call, the same
    events and outcomes as the oracle's fold."""
    c = cached("mirror", lambda: C.ItxCase(mirror_specs()))
    vs = C.validators(4)
    rep = {k: H.Peer("n%d" % k, C.pub_hex(vs[k][1]), "m%d" % k) for k in range(4)}
    known = hashlib.sha256(b"known").digest()
    wevents = []
    for spec, b, s in zip(mirror_specs(), c.bodies, c.signatures):
        wb = sync.WireBody(Transactions=b.Transactions,
                           InternalTransactions=None if b.InternalTransactions is None else [
                               mirror_itx(t) for t in b.InternalTransactions],
                           BlockSignatures=None, CreatorID=spec["c"], OtherParentCreatorID=0, Index=b.Index,
                           SelfParentIndex=7 if spec.get("parents") else -1, OtherParentIndex=-1,
                           Timestamp=b.Timestamp)
        wevents.append(sync.WireEvent(Body=wb, Signature=s))

    def participant_event(pk, index):
        return H.EncodeToString(known)

    stub = OracleVerifier()
    events, outcomes, err = sync.sync_verify_device(wevents, rep, participant_event, stub, fields=True)
    assert err is None and stub.calls == 1 and len(events) == c.n
    st = c.expected()[0]
    for e, (ev, o) in enumerate(zip(events, outcomes)):
        assert ev._hash == c.digests[e].tobytes(), e
        assert o.ok == (st[e] == 1) and o.panic == (st[e] == 3), e
        if st[e] == 2:
            assert o.err == G.event_verify_error(c.bodies[e], c.signatures[e]), e
        if st[e] == 4:
            assert o.err == "invalid signature on internal transaction", e
