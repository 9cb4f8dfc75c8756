"""bv_group_verify_events_itx / bv_group_verify_events_fields on the GPU: the
whole of Event.Verify in one call, sharded by event index across the group's
device slots.  Every group here is made of logical shards of device 0 (one ctx
each): the shard plan, the concurrent per-shard host threads (ITX key decode,
text packing, staging), the rebased kernels (k_itx_body_hash_rb,
k_ev_body_hash_itx_rb, k_ev_body_hash_fields_rb, k_ev_compose_rb) and the bit
merge are the multi-device code path; only the gather is device copies instead
of one RCCL all-gather.

Judges: oracle/gosemantics.py (FieldsCase.expected()) and hashlib for the
digests, exact; a single-context Verifier over the same batch is the second
witness.  Workloads: tests/fields_cases.py."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from babble_amd import events as E
from babble_amd import hashgraph as H
from babble_amd import native, shard
from tests import fields_cases as C

pytestmark = pytest.mark.gpu

_cases = {}


def cached(name, make):
    if name not in _cases:
        _cases[name] = make()
    return _cases[name]


def _bulk(make):
    """make() with BV_SMALL=0 (read at creation): the contexts' host entries
    never take the one-launch small path, whatever the batch's size."""
    old = os.environ.get("BV_SMALL")
    os.environ["BV_SMALL"] = "0"
    try:
        return make()
    finally:
        if old is None:
            del os.environ["BV_SMALL"]
        else:
            os.environ["BV_SMALL"] = old


@pytest.fixture(scope="module")
def g3():
    from babble_amd.verifier import Group

    g = _bulk(lambda: Group([0, 0, 0]))
    yield g
    g.close()


@pytest.fixture(scope="module")
def vbulk():
    from babble_amd.verifier import Verifier

    v = _bulk(lambda: Verifier(0))
    yield v
    v.close()


def mismatch(a, b):
    return np.flatnonzero((a != b).any(axis=1))[:8] if a.shape == b.shape else (a.shape, b.shape)


def check(c, res, what=""):
    """Every output against the oracle's values and hashlib's digests."""
    st, by, ist, bits = c.expected()
    assert np.array_equal(res.msg_hash, c.digests), (what, mismatch(res.msg_hash, c.digests))
    assert np.array_equal(res.itx_hash, c.itx_digests), (what, mismatch(res.itx_hash, c.itx_digests))
    assert np.array_equal(res.itx_status, ist), (what, np.flatnonzero(res.itx_status != ist)[:8])
    assert np.array_equal(res.status, st), (what, np.flatnonzero(res.status != st)[:8], res.status[:16], st[:16])
    assert np.array_equal(res.decided_by, by), (what, np.flatnonzero(res.decided_by != by)[:8])
    assert np.array_equal(res.accept_bits, bits), what


def same_all(a, b, what=""):
    for f in ("msg_hash", "status", "accept_bits", "itx_hash", "itx_status", "decided_by"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


# validators 5 and 6 are no creator of any case: fresh keys (the cases' creators are validators 0..3)
SPECIAL = {0: lambda s: dict(s, itxs=[C.make_itx(1, pubhex="0")]),          # PubKeyHex one byte long: forced REF_PANIC
           1: lambda s: dict(s, signature="1|2|3"),                         # the event signature: REJECT_ERR
           2: lambda s: dict(s, itxs=[C.make_itx(s["c"], netaddr="own")]),  # an ITX whose key equals a creator's
           3: lambda s: dict(s, itxs=[C.make_itx(5 + (s["index"] > 200), netaddr="fresh")])}  # a fresh key


def main_specs():
    """cycle_specs(330) with, in events 130.. (shard 1 of 3; shard 0 of 2) and
    260.. (shard 2 of 3; shard 1 of 2), the four special events."""
    specs = C.cycle_specs(330)
    for base in (130, 260):
        for k, f in SPECIAL.items():
            specs[base + k] = f(specs[base + k])
    return specs


def with_unused_first_hash(p):
    """The same batch with one parent hash no event names in front of the
    table: every shard's hash range, shard 0's too, starts past 0."""
    w = p.ev.events
    ph = np.concatenate([np.full((1, 32), 0x5A, np.uint8), w.parent_hashes])
    ref = np.where(w.parent_kind == E.PARENT_HASH, w.parent_ref + 1, w.parent_ref).astype(np.uint64)
    return dataclasses.replace(p, ev=dataclasses.replace(p.ev, events=dataclasses.replace(w, parent_hashes=ph,
                                                                                           parent_ref=ref)))


def main_case():
    return cached("main", lambda: C.FieldsCase(main_specs()))


def test_three_shards_every_output(g3, vbulk, monkeypatch):
    c = main_case()
    p = with_unused_first_hash(c.packed)
    w = p.ev.events
    st, by, ist, _ = c.expected()
    # what the shards hold, from the oracle's values and the plan, before the device is asked
    dag, bounds, ib, bb, lo, hi = shard.plan_event_fields_shards(w.parent_kind, w.parent_ref, p.ev.itx_start,
                                                                 p.bsig_start, 3)
    assert not dag and bounds == [0, 128, 256, 330]
    for d in range(3):
        a, z = bounds[d], bounds[d + 1]
        assert {0, 1, 4} <= set(st[a:z].tolist()) and (by[a:z] != C.EV_SELF).any() and lo[d] > 0, d
    for base in (130, 260):
        assert (st[base], by[base]) == (3, 0) and ist[int(p.ev.itx_start[base])] == 3  # the forced panic
        assert (st[base + 1], by[base + 1]) == (2, C.EV_SELF)
        assert ist[int(p.ev.itx_start[base + 2])] == 1 and ist[int(p.ev.itx_start[base + 3])] == 1
    assert ib[1] > 0 and bb[1] > 0 and int(w.tx_start[128]) > 0
    assert (p.bsig_val_kind[bb[1]:] == E.BSIG_VAL_BYTES).any()
    monkeypatch.setenv("BV_FIELDS_CHUNK", "64")  # (read per call) chunk bounds inside every shard
    res = g3.verify_events_fields(p)
    check(c, res, "group of 3")
    for d in range(3):
        assert g3.timing(d)["ms_h2d"] > 0, d  # every slot staged: the bulk pipeline
    same_all(res, vbulk.verify_events_fields(p), "single context")
    # without the extra hash slot 0 has no base at all: the un-based kernels beside the rebased ones
    check(c, g3.verify_events_fields(c.packed), "group of 3, shard 0 un-based")


def test_itx_entry_and_no_itx_fields(g3, vbulk):
    c = main_case()
    res = g3.verify_events_itx(c.packed_frag)
    check(c, res, "itx entry")
    same_all(res, vbulk.verify_events_itx(c.packed_frag), "single context")
    n = cached("noitx", lambda: C.FieldsCase(C.cycle_specs(200, itxs=False), itx_fields=False))
    assert n.packed.ev.itx_start is None and n.packed.n_bsig > 100
    res = g3.verify_events_fields(n.packed)
    check(n, res, "no ITX fields")
    assert (res.decided_by == C.EV_SELF).all() and len(res.itx_status) == 0


@pytest.mark.parametrize("n", [1, 64, 100, 130])
def test_tiny_and_empty_shards(g3, n):
    """Shards of (1, 0, 0), (64, 0, 0), (64, 36, 0) and (64, 64, 2) events,
    each on the bulk pipeline of its slot."""
    if n == 1:
        c = cached("one", lambda: C.FieldsCase(
            [dict(C.cycle_specs(130)[13], bsigs=[C.block_sig(1, 0, -2 ** 63), C.block_sig(1, 1, 2 ** 63 - 1, None)])]))
    else:
        c = cached(("cycle", n), lambda: C.FieldsCase(C.cycle_specs(130)[:n]))
    assert c.packed.n_bsig > 0
    check(c, g3.verify_events_fields(c.packed), n)
    assert g3.timing(0)["ms_h2d"] > 0
    check(c, g3.verify_events_itx(c.packed_frag), (n, "itx"))


def test_empty_batch_writes_nothing(g3):
    from babble_amd.verifier import EventItxVerifyResult

    def pattern():
        return EventItxVerifyResult(np.full((1, 32), 0xAA, np.uint8), np.full(1, 0xAA, np.uint8),
                                    np.full(1, 0xAAAA, np.uint64), np.full((1, 32), 0xAA, np.uint8),
                                    np.full(1, 0xAA, np.uint8), np.full(1, 0xAAAA, np.uint32))

    b = E.EventBatchBuilder()
    for fn, batch in ((g3.verify_events_fields_into, b.pack_fields(itx_fields=True)),
                      (g3.verify_events_itx_into, b.pack_itx())):
        out = fn(batch, pattern())  # BV_OK
        for got, want in zip(dataclasses.astuple(out), dataclasses.astuple(pattern())):
            assert np.array_equal(got, want)
    assert len(g3.verify_events_fields(b.pack_fields(itx_fields=True)).status) == 0


def test_unsharded_batches_run_on_slot_0(vbulk):
    from babble_amd.verifier import Group, Verifier

    g, v = Group([0, 0]), Verifier(0)  # default contexts: the one-launch small path is on
    try:
        d = cached("dag", lambda: C.FieldsCase(C.dag_specs()))
        assert (d.packed.ev.events.parent_kind == E.PARENT_EVENT).any()
        res = g.verify_events_fields(d.packed)
        check(d, res, "dag")
        same_all(res, v.verify_events_fields(d.packed), "dag, single context")
        check(d, g.verify_events_itx(d.packed_frag), "dag, itx entry")
        # a batch the default context routes to its one-launch path: nothing is staged on any slot
        s = cached(("cycle", 63), lambda: C.FieldsCase(C.cycle_specs(130)[:63]))
        assert s.packed.n_bsig > 0 and 63 + s.packed.n_itx <= 256
        res = g.verify_events_fields(s.packed)
        check(s, res, "small")
        assert g.timing(0)["ms_h2d"] == 0
        same_all(res, v.verify_events_fields(s.packed), "small, single context")
        # a forward in-batch reference is refused; the next valid call is exact
        w = d.packed.ev.events
        pk, pr = w.parent_kind.copy(), w.parent_ref.copy()
        pk[3, 0], pr[3, 0] = E.PARENT_EVENT, 5
        fwd = dataclasses.replace(d.packed, ev=dataclasses.replace(
            d.packed.ev, events=dataclasses.replace(w, parent_kind=pk, parent_ref=pr)))
        with pytest.raises(native.BvError):
            g.verify_events_fields(fwd)
        check(d, g.verify_events_fields(d.packed), "after the refused batch")
        c = main_case()
        check(c, g.verify_events_fields(c.packed), "bulk, default contexts")
    finally:
        g.close()
        v.close()


def test_pinned_in_place():
    """Inputs from PinnedArena.event_fields_batch, every result array (the
    `out` arrays too) in arena memory."""
    from babble_amd.verifier import EventItxVerifyResult, Group, PinnedArena

    c = main_case()
    n, m = c.n, c.packed.n_itx
    g = _bulk(lambda: Group([0, 0]))
    arena = PinnedArena()
    try:
        res = EventItxVerifyResult(arena.array((n, 32), np.uint8), arena.array(n, np.uint8),
                                   arena.array((n + 63) // 64, np.uint64), arena.array((m, 32), np.uint8),
                                   arena.array(m, np.uint8), arena.array(n, np.uint32))
        for a in dataclasses.astuple(res):
            a[...] = 0xAA
        g.verify_events_fields_into(arena.event_fields_batch(c.packed), res)
        check(c, res, "pinned")
        # any output may be NULL
        part = EventItxVerifyResult(None, res.status, None, None, None, None)
        res.status[...] = 0xAA
        g.verify_events_fields_into(c.packed, part)
        assert np.array_equal(res.status, c.expected()[0])
    finally:
        g.close()
        arena.close()


KC_FIELDS = ("key_path", "kc_hits", "kc_builds", "kc_keys")


def test_key_cache_per_slot():
    from babble_amd.verifier import Group, Verifier

    keys = [pub for _, pub in C.validators(4)]
    plain = cached("plain330", lambda: C.FieldsCase(C.cycle_specs(330)))  # every ITX key is a creator's
    c = main_case()                                                      # and one fresh ITX key per shard
    g = _bulk(lambda: Group([0, 0], flags=native.F_KEY_CACHE))
    v = _bulk(lambda: Verifier(0, flags=native.F_KEY_CACHE))
    try:
        g.register_keys(keys)
        v.register_keys(keys)
        res = g.verify_events_fields(plain.packed)
        for slot in (0, 1):
            t = g.timing(slot)
            assert t["key_path"] == 22 and t["kc_hits"] == 4, (slot, t)
        check(plain, res, "key cache")
        # fresh ITX keys: each slot does what a single key-cache context does with the same shard contents
        res = g.verify_events_fields(c.packed)
        check(c, res, "key cache, fresh ITX keys")
        specs = main_specs()
        for slot, (a, z) in enumerate(((0, 192), (192, 330))):
            part = C.FieldsCase(specs[a:z])
            one = v.verify_events_fields(part.packed)
            assert np.array_equal(one.msg_hash, res.msg_hash[a:z]), mismatch(one.msg_hash, res.msg_hash[a:z])
            tg, tv = g.timing(slot), v.timing()
            assert {k: tg[k] for k in KC_FIELDS} == {k: tv[k] for k in KC_FIELDS}, (slot, tg, tv)
    finally:
        g.close()
        v.close()


def test_argument_errors_then_a_valid_call(g3, vbulk):
    c = main_case()
    p = c.packed

    def text(fn, handle, last_error, batch, patch=None):
        keep = []
        cb = batch.c_struct(keep)
        if patch:
            patch(cb)
        h = np.zeros((p.n_events, 32), np.uint8)
        res = native.BvResult(h.ctypes.data, None, None)
        assert fn(handle, ctypes.byref(cb), ctypes.byref(res), None) == native.BV_E_ARGS
        return last_error(handle).decode()

    L = native.lib()
    bad_start = np.array(p.ev.itx_start, copy=True)
    bad_start[3] = int(bad_start[-1]) + 1  # not monotone
    nonmono = dataclasses.replace(p, ev=dataclasses.replace(p.ev, itx_start=bad_start))
    one = np.ones(4, np.uint64)

    def frag(cb):
        cb.ev.events.itx_off = one.ctypes.data

    for batch, patch, want in ((nonmono, None, "itx_start not monotone"),
                               (p, frag, "events.itx_off / itx_json must be NULL (the ITXs come from fields)")):
        got = text(L.bv_group_verify_events_fields, g3._g, L.bv_group_last_error, batch, patch)
        assert got == want == text(L.bv_verify_events_fields, vbulk._ctx, L.bv_last_error, batch, patch)
    with pytest.raises(native.BvError, match="itx_start not monotone"):
        g3.verify_events_itx(dataclasses.replace(c.packed_frag, itx_start=bad_start))
    check(c, g3.verify_events_fields(p), "after the errors")


def _mirror_events(c):
    return [H.Event(Body=H.EventBody(
        Transactions=b.Transactions, Parents=b.Parents, Creator=b.Creator, Index=b.Index, Timestamp=b.Timestamp,
        InternalTransactions=None if b.InternalTransactions is None else [
            H.InternalTransaction(H.InternalTransactionBody(t.Body.Type, H.Peer(t.Body.Peer.NetAddr, t.Body.Peer.PubKeyHex,
                                                                                t.Body.Peer.Moniker)), t.Signature)
            for t in b.InternalTransactions],
        BlockSignatures=None if b.BlockSignatures is None else [
            H.BlockSignature(t.Validator, t.Index, t.Signature) for t in b.BlockSignatures]), Signature=s)
        for b, s in zip(c.bodies, c.signatures)]


def test_mirror_takes_a_group(g3, vbulk):
    """hashgraph.verify_events(fields=True, group=g): outcome by outcome what
    the same call gives on a Verifier.  The 330-event list is mixed: some
    events carry block signatures, some an empty list, some none (one such
    list goes to bv_group_verify_events_fields whole); the same events
    without any block signature reach bv_group_verify_events_itx."""
    c = main_case()
    kinds = {None if b.BlockSignatures is None else min(len(b.BlockSignatures), 1) for b in c.bodies}
    assert kinds == {None, 0, 1}
    nobsig = cached("nobsig300", lambda: C.FieldsCase([dict(s, bsigs=None) for s in main_specs()[:300]]))
    for case, what in ((c, "fields"), (nobsig, "itx")):
        assert any(b.BlockSignatures is not None for b in case.bodies) == (what == "fields")
        evs, evs1 = _mirror_events(case), _mirror_events(case)
        outs = H.verify_events(evs, fields=True, group=g3)
        ref = H.verify_events(evs1, vbulk, fields=True)
        st = case.expected()[0]
        assert len(outs) == case.n
        for e, (o, r) in enumerate(zip(outs, ref)):
            assert (o.ok, o.err, o.panic) == (r.ok, r.err, r.panic), (what, e)
            assert o.ok == (st[e] == 1) and o.panic == (st[e] == 3), (what, e)
            assert evs[e]._hash == case.digests[e].tobytes() == evs1[e]._hash
    with pytest.raises(ValueError):
        H.verify_events([], group=g3)
