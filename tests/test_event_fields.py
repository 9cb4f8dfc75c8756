"""Whole events from fields on the CPU (babble_amd/csrc/bsigjson.h,
bv_event_itx.cpp's host helpers, the Python mirror).

Judge: oracle/gosemantics.py (EventBody.Marshal with BlockSignatures =
[BlockSignature...], event_status, itx_status) and hashlib; comparisons are
exact.  The serialiser's public form (bv_event_fields_bodies) is compared byte
for byte; the device's streaming sink runs on the host (tests/emu_fields); an
ASan + UBSan driver with its own main fuzzes the emit, length and check
functions.  The GPU half is tests/test_gpu_event_fields.py.  Workloads:
tests/fields_cases.py."""
import ctypes
import dataclasses
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from babble_amd import events as E
from babble_amd import hashgraph as H
from babble_amd import native, sync
from oracle import gosemantics as G
from tests import fields_cases as C
from tests.emu_fields import emu_fields

_cases = {}


def cached(name, make):
    if name not in _cases:
        _cases[name] = make()
    return _cases[name]


def cycle_case():
    return cached("cycle", lambda: C.FieldsCase(C.cycle_specs(130)))


def check_bodies(c):
    """bv_event_fields_bodies == the oracle, len == bytes emitted == that, and
    the EvjSha sink on the CPU gives sha256(oracle body)."""
    p = c.packed
    assert not (p.ev.events.parent_kind == E.PARENT_EVENT).any()
    got = p.event_bodies()
    for e, (g, want) in enumerate(zip(got, c.raw)):
        assert g == want, e
    lens, emitted = emu_fields.lens(p, 1)
    assert lens.tolist() == emitted.tolist() == [len(r) for r in c.raw]
    flat = [t for b in c.bodies for t in (b.BlockSignatures or [])]
    lens, emitted = emu_fields.lens(p, 0)
    assert lens.tolist() == emitted.tolist() == [len(t.json()) for t in flat]
    assert np.array_equal(emu_fields.ev_body_hash(p), c.digests)


def test_cycle_cases_equal_the_oracle():
    c = cycle_case()
    p = c.packed
    shapes = {(None if b.InternalTransactions is None else len(b.InternalTransactions),
               None if b.BlockSignatures is None else len(b.BlockSignatures)) for b in c.bodies}
    assert len(shapes) == 25  # nil / [] / 1 / 2 / 3 of both lists, every combination
    idx = set(p.bsig_index.tolist())
    assert {0, -1, 2 ** 63 - 1, -2 ** 63} <= idx
    assert set(p.bsig_val_kind.tolist()) == {0, 1, 2}
    assert all(re.fullmatch(r"[0-9a-z]+\|[0-9a-z]+", t.Signature)  # real r|s texts
               for b in c.bodies for t in (b.BlockSignatures or []))
    check_bodies(c)


def test_cycle_without_itx_fields():
    """ev.itx_start == NULL: null, or [] where itx_list_nil[e] == 0."""
    c = cached("cycle_noitx", lambda: C.FieldsCase(C.cycle_specs(60, itxs=False), itx_fields=False))
    assert c.packed.ev.itx_start is None and c.packed.ev.itx_list_nil is not None
    assert {b.InternalTransactions is None for b in c.bodies} == {True, False}
    check_bodies(c)
    allnil = cached("allnil", lambda: C.FieldsCase([dict(s, itxs=None) for s in C.cycle_specs(30, itxs=False)],
                                                   itx_fields=None))
    assert allnil.packed.ev.itx_start is None and allnil.packed.ev.itx_list_nil is None
    check_bodies(allnil)


def test_string_grid_as_the_signature():
    c = cached("grid", lambda: C.FieldsCase(C.signature_specs(C.string_grid())))
    assert c.n == 2345
    check_bodies(c)


def test_validator_lengths_nil_validators_nil_and_empty_lists():
    c = cached("validators", lambda: C.FieldsCase(C.validator_specs()))
    p = c.packed
    assert np.diff(p.bsig_val_off)[:7].tolist() == [0, 1, 2, 3, 64, 65, 66]
    assert set(p.bsig_val_kind.tolist()) == {0, 1, 2}
    assert b'"Validator":null' in c.raw[7] and b'"Validator":""' in c.raw[7] and b'"Validator":""' in c.raw[0]
    assert c.raw[8].count(b'"BlockSignatures":null') == 1 and c.raw[9].count(b'"BlockSignatures":[]') == 1
    check_bodies(c)


def test_streaming_sink_at_every_padding_residue():
    c = cached("residues", lambda: C.FieldsCase(C.residue_specs()))
    assert len({len(r) % 64 for r in c.raw}) == 64
    assert {55, 56, 63, 0} <= {len(r) % 64 for r in c.raw}
    check_bodies(c)


def test_dag_bodies_and_parent_positions():
    """In-batch parents: the placeholder form, the positions before the block
    signatures' text and after the ITXs'."""
    c = cached("dag", lambda: C.FieldsCase(C.dag_specs()))
    p = c.packed
    k = p.ev.events.parent_kind
    assert c.n == 40 and (k == E.PARENT_EVENT).any()
    got = p.event_bodies()
    zero = "0" * 64
    for e, (g, body) in enumerate(zip(got, c.bodies)):
        ps = [("0X" + zero) if k[e, j] == E.PARENT_EVENT else s for j, s in enumerate(body.Parents)]
        assert g == dataclasses.replace(body, Parents=ps).Marshal(), e
        pp = emu_fields.ppos(p, e)
        for j in range(2):
            if k[e, j] == E.PARENT_EVENT:
                assert body.BlockSignatures, e  # (the case puts them on these events)
                assert g[pp[j] - 3:pp[j]] == b'"0X' and g[pp[j]:pp[j] + 64] == zero.encode(), (e, j)
                assert g.index(b',"Parents":[') < pp[j] < g.index(b',"BlockSignatures":'), (e, j)
            else:
                assert pp[j] == 0xFFFFFFFF, (e, j)


def test_sanitizer_fuzz_driver():
    exe = emu_fields.fuzz_exe()
    for seed in (1, 2, 3):
        r = subprocess.run([exe, str(seed), "150"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), (seed, r.stdout[-400:], r.stderr[-2000:])
        assert r.stderr == "", r.stderr[-2000:]
        assert int(r.stdout.split()[3]) == 15, r.stdout  # every refusal text of the argument table
    # every batch is refused in every way: one round is enough for all 15
    r = subprocess.run([exe, "5", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and int(r.stdout.split()[3]) == 15, (r.stdout, r.stderr[-2000:])


def test_host_helper_argument_checks():
    L = native.lib()
    p = cycle_case().packed
    off = np.zeros(p.n_events + 1, np.uint64)
    out = np.zeros(1 << 20, np.uint8)

    def call(fb, patch=None):
        keep = []
        cb = fb.c_struct(keep)
        if patch:
            patch(cb)
        return L.bv_event_fields_body_lens(ctypes.byref(cb), off.ctypes.data)

    def arr(a, i, v):
        a = np.array(a, copy=True)
        a[i] = v
        return a

    bad = native.BV_E_ARGS
    assert call(p) == native.BV_OK
    assert L.bv_event_fields_body_lens(None, off.ctypes.data) == bad
    one = np.ones(4, np.uint64)
    assert call(p, lambda cb: setattr(cb.ev.events, "bsig_off", one.ctypes.data)) == bad
    assert call(p, lambda cb: setattr(cb.ev.events, "bsig_json", one.ctypes.data)) == bad
    assert call(p, lambda cb: setattr(cb.ev.events, "itx_off", one.ctypes.data)) == bad
    assert call(p, lambda cb: setattr(cb, "bsig_start", None)) == bad
    assert call(dataclasses.replace(p, bsig_start=arr(p.bsig_start, 0, 1))) == bad
    assert call(dataclasses.replace(p, bsig_start=arr(p.bsig_start, 4, 10 ** 6))) == bad
    assert call(dataclasses.replace(p, bsig_start=arr(p.bsig_start, -1, (1 << 32) + 1))) == bad
    assert call(p, lambda cb: setattr(cb, "bsig_index", None)) == bad
    assert call(p, lambda cb: setattr(cb, "bsig_sig_off", None)) == bad
    assert call(dataclasses.replace(p, bsig_sig_off=arr(p.bsig_sig_off, 0, 1))) == bad
    assert call(dataclasses.replace(p, bsig_sig_off=arr(p.bsig_sig_off, 1, 10 ** 9))) == bad
    assert call(p, lambda cb: setattr(cb, "bsig_sig", None)) == bad
    assert call(dataclasses.replace(p, bsig_val_kind=arr(p.bsig_val_kind, 5, 3))) == bad
    assert call(p, lambda cb: setattr(cb, "bsig_val_off", None)) == bad
    assert call(dataclasses.replace(p, bsig_val_off=arr(p.bsig_val_off, 1, 10 ** 9))) == bad
    assert call(p, lambda cb: setattr(cb, "bsig_val_bytes", None)) == bad
    assert call(dataclasses.replace(p, ev=dataclasses.replace(p.ev, itx_start=arr(p.ev.itx_start, 0, 1)))) == bad
    # bodies: offsets too short for a body, a NULL output
    assert call(p) == native.BV_OK
    keep = []
    cb = p.c_struct(keep)
    assert L.bv_event_fields_bodies(ctypes.byref(cb), off.ctypes.data, out.ctypes.data) == native.BV_OK
    assert L.bv_event_fields_bodies(ctypes.byref(cb), off.ctypes.data, None) == bad
    short = off.copy()
    short[1:] -= 1
    assert L.bv_event_fields_bodies(ctypes.byref(cb), short.ctypes.data, out.ctypes.data) == bad


def test_abi_version_and_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "babbleverify.h")).read()
    assert re.search(r"#define\s+BV_ABI_VERSION\s+6\b", header)
    L = native.lib()
    assert L.bv_abi_version() == 6
    for name in ("bv_verify_events_fields", "bv_event_fields_body_lens", "bv_event_fields_bodies"):
        assert name in native.EXPORTS and name in header
        assert getattr(L, name).restype is ctypes.c_int
    for name, v in (("BV_BSIG_VAL_CREATOR", 0), ("BV_BSIG_VAL_BYTES", 1), ("BV_BSIG_VAL_NIL", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, v), header)
    assert (E.BSIG_VAL_CREATOR, E.BSIG_VAL_BYTES, E.BSIG_VAL_NIL) == (0, 1, 2)


# ----------------------------------------------------------------------------
# the Python mirror over a stub verifier that answers from the oracle
# ----------------------------------------------------------------------------
class OracleVerifier:
    """verify_events_fields / verify_events_itx / verify answered by the
    oracle from the packed batch alone (event bodies through the library's
    host serialiser; no device)."""

    def __init__(self):
        self.calls = []

    def _events(self, xb, bodies):
        from babble_amd.verifier import EventItxVerifyResult

        n, m = xb.n_events, xb.n_itx
        ev = xb.events
        assert not (ev.parent_kind == E.PARENT_EVENT).any()
        so, raw = xb.itx_str_off, xb.itx_str.tobytes()
        strs = [raw[int(so[k]):int(so[k + 1])] for k in range(4 * m)]
        sigs = [ev.sig_text.tobytes()[int(ev.sig_off[e]):int(ev.sig_off[e + 1])] for e in range(n)]
        keys = [ev.key_bytes.tobytes()[int(ev.key_off[k]):int(ev.key_off[k + 1])] for k in range(len(ev.key_off) - 1)]
        ist = [G.itx_status(G.InternalTransaction(
            G.InternalTransactionBody(int(xb.itx_type[i]), G.Peer(*strs[4 * i:4 * i + 3])), strs[4 * i + 3]))
            for i in range(m)]
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
        return EventItxVerifyResult(h, np.array(st, np.uint8), np.zeros((n + 63) // 64, np.uint64),
                                    np.zeros((m, 32), np.uint8), np.array(ist, np.uint8), np.array(by, np.uint32))

    def verify_events_fields(self, fb):
        self.calls.append("fields")
        assert fb.ev.events.bsig_off is None and fb.ev.events.itx_off is None  # no JSON from the caller
        return self._events(fb.ev, fb.event_bodies())

    def verify_events_itx(self, xb):
        self.calls.append("itx")
        return self._events(xb, xb.event_bodies())

    def verify(self, packed):  # the fields=False route: the C oracle over the serialised bodies
        import types

        from oracle import coracle

        self.calls.append("batch")
        h, st, _ = coracle.verify_batch(packed.as_dict())
        return types.SimpleNamespace(status=st, msg_hash=h)


def mirror_itx(t):
    return H.InternalTransaction(H.InternalTransactionBody(t.Body.Type, H.Peer(t.Body.Peer.NetAddr, t.Body.Peer.PubKeyHex,
                                                                             t.Body.Peer.Moniker)), t.Signature)


def mirror_events(c):
    return [H.Event(Body=H.EventBody(
        Transactions=b.Transactions, Parents=b.Parents, Creator=b.Creator, Index=b.Index, Timestamp=b.Timestamp,
        InternalTransactions=None if b.InternalTransactions is None else [mirror_itx(t) for t in b.InternalTransactions],
        BlockSignatures=None if b.BlockSignatures is None else [
            H.BlockSignature(t.Validator, t.Index, t.Signature) for t in b.BlockSignatures]),
        Signature=s) for b, s in zip(c.bodies, c.signatures)]


def test_mirror_takes_the_fields_entry_and_serialises_nothing(monkeypatch):
    c = cached("mirror", lambda: C.FieldsCase(C.cycle_specs(50)))
    st = c.expected()[0]
    assert {0, 1, 4} <= set(st.tolist())
    stub = OracleVerifier()
    evs = mirror_events(c)
    monkeypatch.setattr(H.J, "slice_", lambda *a, **k: pytest.fail("J.slice_ called with fields=True"))
    outs = H.verify_events(evs, stub, fields=True)
    assert stub.calls == ["fields"]
    for e, o in enumerate(outs):
        assert o.ok == (st[e] == 1) and o.panic == (st[e] == 3), e
        assert evs[e]._hash == c.digests[e].tobytes(), e
    monkeypatch.undo()
    # the same outcomes and hashes as the fields=False route over the serialised bodies
    evs2 = mirror_events(c)
    outs2 = H.verify_events(evs2, stub, fields=False)
    assert stub.calls == ["fields", "batch"]
    for e, (o, o2) in enumerate(zip(outs, outs2)):
        assert (o.ok, o.err, o.panic) == (o2.ok, o2.err, o2.panic), e
        assert evs[e]._hash == evs2[e]._hash, e
    # events without block signatures make exactly the call they made before
    plain = cached("plain", lambda: C.FieldsCase([dict(s, bsigs=None) for s in C.cycle_specs(10)]))
    stub2 = OracleVerifier()
    H.verify_events(mirror_events(plain), stub2, fields=True)
    assert stub2.calls == ["itx"]


def test_sync_fields_takes_the_fields_entry(monkeypatch):
    """sync_verify_device(fields=True) with BlockSignatures on the wire: one
    verify_events_fields call, no J.slice_, the oracle's hashes and fold."""
    specs = C.cycle_specs(30)
    for s in specs:  # WireEvent.BlockSignatures: the Validator is always the creator
        s["parents"] = [("hash", hashlib.sha256(b"known").digest()), None]
        s["bsigs"] = None if s["bsigs"] is None else [C.block_sig(s["c"], t.Index & 0xFF, t.Index, signature=t.Signature)
                                                      for t in s["bsigs"]]
    c = C.FieldsCase(specs)
    vs = C.validators(4)
    rep = {k: H.Peer("n%d" % k, "0X" + vs[k][1].hex().upper(), "m%d" % k) for k in range(4)}
    wevents = []
    for spec, b, s in zip(specs, c.bodies, c.signatures):
        wb = sync.WireBody(Transactions=b.Transactions,
                           InternalTransactions=None if b.InternalTransactions is None else [
                               mirror_itx(t) for t in b.InternalTransactions],
                           BlockSignatures=None if b.BlockSignatures is None else [
                               sync.WireBlockSignature(t.Index, t.Signature) for t in b.BlockSignatures],
                           CreatorID=spec["c"], OtherParentCreatorID=0, Index=b.Index, SelfParentIndex=7,
                           OtherParentIndex=-1, Timestamp=b.Timestamp)
        wevents.append(sync.WireEvent(Body=wb, Signature=s))
    stub = OracleVerifier()
    monkeypatch.setattr(sync.J, "slice_", lambda *a, **k: pytest.fail("J.slice_ called with fields=True"))
    events, outcomes, err = sync.sync_verify_device(wevents, rep, lambda pk, index: H.EncodeToString(
        hashlib.sha256(b"known").digest()), stub, fields=True)
    assert err is None and stub.calls == ["fields"] and len(events) == c.n
    st = c.expected()[0]
    for e, (ev, o) in enumerate(zip(events, outcomes)):
        assert ev._hash == c.digests[e].tobytes(), e
        assert o.ok == (st[e] == 1) and o.panic == (st[e] == 3), e
