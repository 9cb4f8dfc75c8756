"""bv_verify_events_fields on the device: a whole Event from fields, the
BlockSignatures member included (k_ev_body_hash_fields;
babble_amd/csrc/bsigjson.h), on the bulk, DAG and one-launch routes.

Judge: oracle/gosemantics.py (EventBody.Marshal with BlockSignatures =
[BlockSignature...], itx_status, event_status) and hashlib for the digests;
comparisons are exact.  Every event and every ITX of every batch is compared.
Workloads: tests/fields_cases.py."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from babble_amd import events as E
from babble_amd import native
from babble_amd.verifier import Verifier
from tests import fields_cases as C

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


def mismatch(a, b):
    return np.flatnonzero((a != b).any(axis=1))[:8] if a.shape == b.shape else (a.shape, b.shape)


def check(c, res, what=""):
    st, by, ist, bits = c.expected()
    assert np.array_equal(res.msg_hash, c.digests), (what, mismatch(res.msg_hash, c.digests))
    assert np.array_equal(res.itx_hash, c.itx_digests), (what, mismatch(res.itx_hash, c.itx_digests))
    assert np.array_equal(res.itx_status, ist), (what, np.flatnonzero(res.itx_status != ist)[:8])
    assert np.array_equal(res.status, st), (what, np.flatnonzero(res.status != st)[:8], res.status[:16], st[:16])
    assert np.array_equal(res.decided_by, by), (what, np.flatnonzero(res.decided_by != by)[:8])
    assert np.array_equal(res.accept_bits, bits), what


def same(a, b):
    assert np.array_equal(a.msg_hash, b.msg_hash) and np.array_equal(a.status, b.status)
    assert np.array_equal(a.accept_bits, b.accept_bits)


def cycle_case(n):
    return cached(("cycle", n), lambda: C.FieldsCase(C.cycle_specs(130)[:n]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_lane_and_word_boundaries(vbulk, n):
    """Bulk batches whose block-signature and ITX lists cycle nil / [] / 1 / 2
    / 3 on different periods, valid signatures mixed with corrupted ones (the
    first n events of the 130-event batch): k_ev_body_hash_fields."""
    c = cycle_case(n) if n > 1 else cached("one", lambda: C.FieldsCase(
        [dict(C.cycle_specs(130)[13], bsigs=[C.block_sig(1, 0, -2 ** 63), C.block_sig(1, 1, 2 ** 63 - 1, None)])]))
    assert c.packed.n_bsig > 0
    if n >= 63:
        assert {0, 1, 4} <= set(c.expected()[0].tolist())
    check(c, vbulk.verify_events_fields(c.packed), n)
    assert vbulk.timing()["ms_h2d"] > 0  # staged: the bulk pipeline


@pytest.mark.parametrize("itx_fields", [True, False])
def test_bulk_route_in_chunks_of_64_events(vbulk, monkeypatch, itx_fields):
    """The bulk route's chunked staging (BV_FIELDS_CHUNK, read per call; 2^17
    events by default): 130 events in chunks of 64 + 64 + 2, every array in
    event-range slices, the chunks hashed and verified one after another."""
    c = cycle_case(130) if itx_fields else cached("noitx", lambda: C.FieldsCase(C.cycle_specs(130, itxs=False),
                                                                                  itx_fields=False))
    monkeypatch.setenv("BV_FIELDS_CHUNK", "64")
    check(c, vbulk.verify_events_fields(c.packed), "chunks")
    assert vbulk.timing()["ms_h2d"] > 0
    # the same arrays in pinned memory (arrays this small are still copied into the staging block; slices of
    # 256 KiB and more are read where they lie, which tools/ab_event_fields.py checks against bv_verify_events)
    from babble_amd.verifier import PinnedArena

    arena = PinnedArena()
    try:
        check(c, vbulk.verify_events_fields(arena.event_fields_batch(c.packed)), "chunks, pinned")
    finally:
        arena.close()


def test_chunks_with_one_large_pinned_array(vbulk, monkeypatch):
    """200 events with at least one block signature each, in chunks of 64 + 64
    + 64 + 8, with 300 000 bytes of transactions (past the 256 KiB floor) in
    bv_host_alloc memory and every other array pageable: each chunk's tx_bytes
    slice crosses by DMA from where it lies, the other slices through the
    staging block.  Equal to the oracle and to the all-pageable call; every
    fifth signature is corrupted."""
    import random

    from babble_amd.verifier import PinnedArena

    def make():
        rng = random.Random(5)
        specs = C.cycle_specs(200)
        for e, s in enumerate(specs):
            s["txs"] = [bytes(rng.getrandbits(8) for _ in range(750)) for _ in range(2)]
            if not s["bsigs"]:
                s["bsigs"] = [C.block_sig(s["c"], 1000 + e, e)]
        return C.FieldsCase(specs)

    c = cached("big_tx", make)
    p = c.packed
    assert p.ev.events.tx_bytes.nbytes == 300_000 and p.n_bsig >= 200 and {0, 1, 4} <= set(c.expected()[0].tolist())
    monkeypatch.setenv("BV_FIELDS_CHUNK", "64")
    arena = PinnedArena()
    try:
        events = dataclasses.replace(p.ev.events, tx_bytes=arena.copy(p.ev.events.tx_bytes))
        mixed = dataclasses.replace(p, ev=dataclasses.replace(p.ev, events=events))
        res = vbulk.verify_events_fields(mixed)
        assert vbulk.timing()["ms_h2d"] > 0
        check(c, res, "tx_bytes pinned")
        ref = vbulk.verify_events_fields(p)
        check(c, ref, "pageable")
        same(res, ref)
    finally:
        arena.close()


@pytest.mark.parametrize("n", [3, 63])
def test_small_batches_take_the_one_launch_path(n):
    c = cycle_case(n)
    assert c.packed.n_bsig > 0 and n + c.packed.n_itx <= 256
    v = Verifier(0, flags=native.F_KEY_CACHE)
    try:
        v.register_keys([pub for _, pub in C.validators(4)])
        check(c, v.verify_events_fields(c.packed), n)
        t = v.timing()
        assert t["ms_h2d"] == 0, t
    finally:
        v.close()


@pytest.mark.parametrize("route", ["default", "bulk"])
def test_no_itx_fields_equals_verify_events_over_fragments(v0, vbulk, route):
    """ev.itx_start == NULL, block signatures as fields: the oracle, and bit
    for bit bv_verify_events over the oracle-built bsig_json (and "[]" ITX)
    fragments."""
    v = vbulk if route == "bulk" else v0
    c = cached("noitx", lambda: C.FieldsCase(C.cycle_specs(130, itxs=False), itx_fields=False))
    p = c.packed
    assert p.ev.itx_start is None and p.n_itx == 0 and p.n_bsig > 100
    res = v.verify_events_fields(p)
    check(c, res, route)
    same(res, v.verify_events(c.events_frag()))
    assert (res.decided_by == C.EV_SELF).all()


def test_escapes_on_the_device(vbulk):
    """Every single byte and every lead x trail pair as the Signature of one
    block signature per event: the event digests."""
    c = cached("escapes", lambda: C.FieldsCase(
        C.signature_specs([bytes([b]) for b in range(256)] + C.pair_strings()), itx_fields=None))
    assert c.n == 328
    res = vbulk.verify_events_fields(c.packed)
    assert np.array_equal(res.msg_hash, c.digests), mismatch(res.msg_hash, c.digests)


def test_padding_residues(vbulk):
    c = cached("residues", lambda: C.FieldsCase(C.residue_specs(), itx_fields=None))
    assert len({len(r) % 64 for r in c.raw}) == 64
    res = vbulk.verify_events_fields(c.packed)
    assert np.array_equal(res.msg_hash, c.digests), mismatch(res.msg_hash, c.digests)


@pytest.mark.parametrize("route", ["default", "bulk"])
def test_dag_batch(v0, vbulk, route):
    """40 events of 4 creators, block signatures on the events with in-batch
    parents, ITXs on every fifth: the oracle, and bv_verify_events_itx over the
    same events with oracle-built fragments."""
    v = vbulk if route == "bulk" else v0
    c = cached("dag", lambda: C.FieldsCase(C.dag_specs()))
    k = c.packed.ev.events.parent_kind
    assert c.n == 40 and (k == E.PARENT_EVENT).sum() > 60 and c.packed.n_itx == 8 and c.packed.n_bsig > 60
    assert all(bool(b.BlockSignatures) == bool((k[e] == E.PARENT_EVENT).any()) for e, b in enumerate(c.bodies))
    res = v.verify_events_fields(c.packed)
    check(c, res, route)
    ref = v.verify_events_itx(c.packed_frag)
    same(res, ref)
    assert np.array_equal(res.itx_hash, ref.itx_hash) and np.array_equal(res.itx_status, ref.itx_status)
    assert np.array_equal(res.decided_by, ref.decided_by)


def test_no_block_signature_equals_verify_events_itx(v0):
    """n_bsig == 0 (nil and empty lists): bv_verify_events_itx's results over
    the same batch with nil / [] fragments."""
    specs = [dict(s, bsigs=None if e % 2 else []) for e, s in enumerate(C.cycle_specs(70))]
    c = cached("nobsig", lambda: C.FieldsCase(specs))
    assert c.packed.n_bsig == 0 and c.packed.n_itx > 0
    res = v0.verify_events_fields(c.packed)
    check(c, res, "no bsig")
    ref = v0.verify_events_itx(c.packed_frag)
    same(res, ref)
    assert np.array_equal(res.itx_hash, ref.itx_hash) and np.array_equal(res.itx_status, ref.itx_status)
    assert np.array_equal(res.decided_by, ref.decided_by)
    # and without ITX fields: bv_verify_events
    specs2 = [dict(s, bsigs=None if e % 2 else [], itxs=None if e % 3 else []) for e, s in enumerate(C.cycle_specs(70))]
    c2 = cached("nothing", lambda: C.FieldsCase(specs2, itx_fields=False))
    assert c2.packed.ev.itx_start is None
    res2 = v0.verify_events_fields(c2.packed)
    check(c2, res2, "no bsig, no itx fields")
    same(res2, v0.verify_events(c2.events_frag()))


def test_argument_errors_then_a_valid_call(v0):
    c = cycle_case(65)
    p = c.packed
    nb = p.n_bsig
    assert nb > 0 and (p.bsig_val_kind == E.BSIG_VAL_BYTES).any()

    def bad(fb=None, patch=None):
        keep = []
        cb = (fb or p).c_struct(keep)
        if patch:
            patch(cb)
        h = np.zeros((p.n_events, 32), np.uint8)
        res = native.BvResult(h.ctypes.data, None, None)
        rc = v0._L.bv_verify_events_fields(v0._ctx, ctypes.byref(cb), ctypes.byref(res), None)
        assert rc == native.BV_E_ARGS, rc
        assert v0._L.bv_last_error(v0._ctx)

    def rep(**kw):
        return dataclasses.replace(p, **kw)

    def rep_ev(**kw):
        return dataclasses.replace(p, ev=dataclasses.replace(p.ev, **kw))

    def arr(a, i, v):
        a = np.array(a, copy=True)
        a[i] = v
        return a

    one = np.ones(4, np.uint64)
    # what bv_verify_events_itx rejects
    bad(patch=lambda cb: setattr(cb.ev.events, "itx_off", one.ctypes.data))
    bad(patch=lambda cb: setattr(cb.ev.events, "itx_json", one.ctypes.data))
    bad(patch=lambda cb: setattr(cb.ev.events, "sig_text", None))
    bad(rep_ev(itx_start=arr(p.ev.itx_start, 0, 1)))
    bad(rep_ev(itx_start=arr(p.ev.itx_start, 3, int(p.ev.itx_start[-1]) + 1)))
    bad(patch=lambda cb: setattr(cb.ev, "itx_str_off", None))
    bad(rep_ev(itx_str_off=arr(p.ev.itx_str_off, 2, int(p.ev.itx_str_off[-1]) + 1)))
    bad(patch=lambda cb: setattr(cb.ev, "itx_str", None))
    bad(patch=lambda cb: setattr(cb.ev, "itx_type", None))
    bad(rep_ev(events=dataclasses.replace(p.ev.events, creator=arr(p.ev.events.creator, 5, 99))))
    pk, pr = arr(p.ev.events.parent_kind, (0, 0), E.PARENT_EVENT), arr(p.ev.events.parent_ref, (0, 0), 0)
    bad(rep_ev(events=dataclasses.replace(p.ev.events, parent_kind=pk, parent_ref=pr)))
    # the block-signature fields
    bad(patch=lambda cb: setattr(cb.ev.events, "bsig_off", one.ctypes.data))
    bad(patch=lambda cb: setattr(cb.ev.events, "bsig_json", one.ctypes.data))
    bad(patch=lambda cb: setattr(cb, "bsig_start", None))
    bad(rep(bsig_start=arr(p.bsig_start, 0, 1)))
    bad(rep(bsig_start=arr(p.bsig_start, 3, nb + 1)))
    huge = np.zeros_like(p.bsig_start)
    huge[-1] = (1 << 32) + 1  # n_bsig > 2^32 (nothing past bsig_start is read)
    bad(rep(bsig_start=huge))
    bad(patch=lambda cb: setattr(cb, "bsig_index", None))
    bad(patch=lambda cb: setattr(cb, "bsig_sig_off", None))
    bad(rep(bsig_sig_off=arr(p.bsig_sig_off, 0, 1)))
    bad(rep(bsig_sig_off=arr(p.bsig_sig_off, 2, int(p.bsig_sig_off[-1]) + 1)))
    bad(patch=lambda cb: setattr(cb, "bsig_sig", None))
    bad(rep(bsig_val_kind=arr(p.bsig_val_kind, 1, 3)))
    bad(patch=lambda cb: setattr(cb, "bsig_val_off", None))
    bad(rep(bsig_val_off=arr(p.bsig_val_off, 2, int(p.bsig_val_off[-1]) + 1)))
    bad(patch=lambda cb: setattr(cb, "bsig_val_bytes", None))
    check(c, v0.verify_events_fields(p), "after the errors")
