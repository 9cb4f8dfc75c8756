"""Host side of bv_group_verify_events_itx / bv_group_verify_events_fields, no
device: the shard plan (bv_plan_event_fields_shards against its restatement in
babble_amd/shard.py, its properties, and the same cases through an ASan +
UBSan build of hostplan.cpp in a stand-alone driver run as a subprocess), the
rebased ITX / fields serialisers and the rebased fold on the host, given only
a shard's slices and its bases (tests/emu_fieldshards), against hashlib over
the oracle's bodies and the oracle's outcomes, and the new symbols."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from babble_amd import events as E
from babble_amd import native, shard
from babble_amd.verifier import plan_event_fields_shards
from oracle import gosemantics as G
from tests.emu_fieldshards import emu_fieldshards as emu
from tests.fields_cases import FieldsCase, cycle_specs, make_itx


# ---------------------------------------------------------------------------
# The plan
# ---------------------------------------------------------------------------
def _cases():
    """1,000 random (D, n_parent_hashes, kinds[n, 2], refs[n, 2], itx_start or
    None, bsig_start): n in [0, 700], D in [1, 9], 0..3 ITXs and 0..3 block
    signatures per event, every third case without itx_start, every second
    with at least one in-batch (EVENT) parent when it has two events."""
    rng = np.random.default_rng(43)
    out = []
    for t in range(1000):
        n = int(rng.integers(0, 701))
        D = int(rng.integers(1, 10))
        nh = int(rng.integers(0, 51))
        kinds = rng.integers(0, 2 if nh else 1, size=(n, 2)).astype(np.uint8)
        refs = np.where(kinds == 1, rng.integers(0, max(nh, 1), size=(n, 2)), 0).astype(np.uint64)
        if t % 2 and n >= 2:
            for e in rng.integers(1, n, size=int(rng.integers(1, 6))):
                p = int(rng.integers(0, 2))
                kinds[e, p] = E.PARENT_EVENT
                refs[e, p] = int(rng.integers(0, e))

        def starts():
            s = np.zeros(n + 1, np.uint64)
            s[1:] = np.cumsum(rng.integers(0, 4, size=n))
            return s

        out.append((D, nh, kinds, refs, None if t % 3 == 2 else starts(), starts()))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _c_plan(D, nh, kinds, refs, itx_start, bsig_start):
    kinds = np.ascontiguousarray(kinds, np.uint8)
    refs = np.ascontiguousarray(refs, np.uint64)
    f = E.BvEventFieldsBatch()
    b = f.ev.events
    b.n_events = len(kinds)
    b.n_parent_hashes = nh
    # (never NULL: an empty batch still passes valid pointers)
    b.parent_kind = kinds.ctypes.data if kinds.size else np.zeros(1, np.uint8).ctypes.data
    b.parent_ref = refs.ctypes.data if refs.size else np.zeros(1, np.uint64).ctypes.data
    f.ev.itx_start = None if itx_start is None else itx_start.ctypes.data
    f.bsig_start = bsig_start.ctypes.data
    eb, ib, bb = (np.zeros(D + 1, np.uint64) for _ in range(3))
    lo, hi = np.zeros(D, np.uint64), np.zeros(D, np.uint64)
    rc = native.lib().bv_plan_event_fields_shards(ctypes.addressof(f), D, eb.ctypes.data, ib.ctypes.data,
                                                  bb.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    return rc, eb.tolist(), ib.tolist(), bb.tolist(), lo.tolist(), hi.tolist()


def _c_event_plan(D, nh, kinds, refs):
    b = E.BvEventBatch()
    b.n_events = len(kinds)
    b.n_parent_hashes = nh
    b.parent_kind = kinds.ctypes.data if kinds.size else np.zeros(1, np.uint8).ctypes.data
    b.parent_ref = refs.ctypes.data if refs.size else np.zeros(1, np.uint64).ctypes.data
    eb, lo, hi = np.zeros(D + 1, np.uint64), np.zeros(D, np.uint64), np.zeros(D, np.uint64)
    rc = native.lib().bv_plan_event_shards(ctypes.addressof(b), D, eb.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    return rc, eb.tolist(), lo.tolist(), hi.tolist()


def test_plan_c_equals_model_and_properties(cases):
    n_dag = n_noitx = 0
    for D, nh, kinds, refs, its, bss in cases:
        rc, eb, ib, bb, lo, hi = _c_plan(D, nh, kinds, refs, its, bss)
        dag, mb, mib, mbb, mlo, mhi = shard.plan_event_fields_shards(kinds, refs, its, bss, D)
        assert (rc, eb, ib, bb, lo, hi) == (int(dag), mb, mib, mbb, mlo, mhi)
        # the event bounds and hash ranges are bv_plan_event_shards'
        assert (rc, eb, lo, hi) == _c_event_plan(D, nh, kinds, refs)
        # the ITX and block-signature bounds are the starts at those events
        assert ib == ([0] * (D + 1) if its is None else [int(its[e]) for e in eb])
        assert bb == [int(bss[e]) for e in eb]
        n = len(kinds)
        if np.any(kinds == E.PARENT_EVENT):  # a DAG batch is whole on shard 0
            assert rc == 1 and eb == [0] + [n] * D
            assert bb == [0] + [int(bss[n])] * D
        n_dag += rc
        n_noitx += its is None
    assert 400 < n_dag < 600 and 300 < n_noitx < 360


def test_plan_fixed_cases():
    def plan(n, D, per_itx=1, per_bsig=2):
        kinds = np.zeros((n, 2), np.uint8)
        its = np.arange(n + 1, dtype=np.uint64) * per_itx
        bss = np.arange(n + 1, dtype=np.uint64) * per_bsig
        return _c_plan(D, 0, kinds, np.zeros((n, 2), np.uint64), its, bss)

    assert plan(100, 3) == (0, [0, 64, 100, 100], [0, 64, 100, 100], [0, 128, 200, 200], [0] * 3, [0] * 3)
    assert plan(130, 3) == (0, [0, 64, 128, 130], [0, 64, 128, 130], [0, 128, 256, 260], [0] * 3, [0] * 3)
    assert plan(0, 2) == (0, [0, 0, 0], [0, 0, 0], [0, 0, 0], [0] * 2, [0] * 2)
    assert plan(1, 8) == (0, [0] + [1] * 8, [0] + [1] * 8, [0] + [2] * 8, [0] * 8, [0] * 8)
    # a shard whose events own no ITX between shards that do; hash ranges; no itx_start
    kinds = np.zeros((200, 2), np.uint8)
    refs = np.zeros((200, 2), np.uint64)
    for e, r in ((3, 7), (60, 2), (64, 9), (199, 40)):
        kinds[e, 1], refs[e, 1] = E.PARENT_HASH, r
    its = np.zeros(201, np.uint64)
    its[1:] = np.cumsum([2 if e < 64 or e >= 128 else 0 for e in range(200)])
    bss = np.arange(201, dtype=np.uint64)
    assert _c_plan(4, 41, kinds, refs, its, bss) == (0, [0, 64, 128, 192, 200], [0, 128, 128, 256, 272],
                                                     [0, 64, 128, 192, 200], [2, 9, 0, 40], [8, 10, 0, 41])
    assert _c_plan(4, 41, kinds, refs, None, bss)[2] == [0] * 5
    kinds[100, 0], refs[100, 0] = E.PARENT_EVENT, 99  # a DAG batch: whole on shard 0
    assert _c_plan(3, 41, kinds, refs, its, bss) == (1, [0, 200, 200, 200], [0, 272, 272, 272], [0, 200, 200, 200],
                                                     [2, 0, 0], [41, 0, 0])


def test_plan_bad_arguments():
    L = native.lib()
    kinds = np.array([[1, 0], [0, 1]], np.uint8)
    refs = np.array([[4, 0], [0, 5]], np.uint64)
    s = np.arange(3, dtype=np.uint64)
    assert _c_plan(2, 6, kinds, refs, s, s)[0] == 0
    assert _c_plan(2, 5, kinds, refs, s, s)[0] == native.BV_E_ARGS  # a HASH ref >= n_parent_hashes
    kinds[0, 0] = 3
    assert _c_plan(2, 6, kinds, refs, s, s)[0] == native.BV_E_ARGS  # an unknown parent kind
    f = E.BvEventFieldsBatch()
    x = np.zeros(4, np.uint64)
    p = x.ctypes.data
    fp = ctypes.addressof(f)
    assert L.bv_plan_event_fields_shards(None, 2, p, p, p, p, p) == native.BV_E_ARGS
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert L.bv_plan_event_fields_shards(fp, 2, *args) == native.BV_E_ARGS
    assert L.bv_plan_event_fields_shards(fp, 0, p, p, p, p, p) == native.BV_E_ARGS
    assert L.bv_plan_event_fields_shards(fp, -3, p, p, p, p, p) == native.BV_E_ARGS
    assert L.bv_plan_event_fields_shards(fp, 2, p, p, p, p, p) == 0  # an empty batch needs no start array


def test_plan_fuzz_sanitized(cases):
    """The same random cases through hostplan.cpp built with ASan + UBSan, each
    copied into exactly-sized heap buffers by the stand-alone driver."""
    exe = emu.plan_exe()

    def row(a):
        return ",".join(map(str, np.asarray(a).reshape(-1).tolist())) or "-"

    lines = []
    for D, nh, kinds, refs, its, bss in cases:
        ks = "".join(map(str, kinds.reshape(-1).tolist())) or "-"
        lines.append(f"P {D} {len(kinds)} {nh} {ks} {row(refs)} {'-' if its is None else row(its)} {row(bss)}")
    lines += ["P 2 2 5 1001 4,0,0,5 0,1,2 0,0,3", "P 2 2 6 1001 4,0,0,5 0,1,2 0,0,3", "P 1 1 3 30 0,0 0,1 0,1", "N"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    for (D, nh, kinds, refs, its, bss), line in zip(cases, out):
        f = line.split()
        dag, *want = shard.plan_event_fields_shards(kinds, refs, its, bss, D)
        assert f[0] == "P" and int(f[1]) == int(dag)
        assert [[int(x) for x in g.split(",")] for g in f[2:]] == [list(w) for w in want]
    assert out[-4] == "P -1"  # a HASH ref >= n_parent_hashes: refused
    assert out[-3] == "P 0 0,2,2 0,2,2 0,3,3 4,0 6,0"
    assert out[-2] == "P -1"  # an unknown parent kind
    assert out[-1] == "N -1 -1 -1 -1 -1 -1 -1 -1"


def test_plan_python_binding():
    c = _case200()
    dag, eb, ib, bb, lo, hi = plan_event_fields_shards(c.packed, 4)
    w = c.packed.ev.events
    want = shard.plan_event_fields_shards(w.parent_kind, w.parent_ref, c.packed.ev.itx_start, c.packed.bsig_start, 4)
    assert (dag, eb.tolist(), ib.tolist(), bb.tolist(), lo.tolist(), hi.tolist()) == want and not dag
    assert eb.tolist() == [0, 64, 128, 192, 200]


# ---------------------------------------------------------------------------
# The rebased serialisers and the rebased fold, given only a shard's slices
# ---------------------------------------------------------------------------
_CASES = {}


def _case200() -> FieldsCase:
    if "c200" not in _CASES:
        specs = cycle_specs(200)
        for e in (70, 140, 195):  # in shards 1, 2 and 3 of 4: an ITX whose PubKeyHex is one byte long, then the event's own
            specs[e]["itxs"] = [make_itx(1, pubhex="0")] + (specs[e]["itxs"] or [])
        _CASES["c200"] = FieldsCase(specs)
    return _CASES["c200"]


def _shards(w, D):
    dag, bounds, lo, hi = shard.plan_event_shards(w.parent_kind, w.parent_ref, D)
    assert not dag
    return [(bounds[d], bounds[d + 1], lo[d], hi[d]) for d in range(D)]


def _check_bodies(c: FieldsCase, D: int):
    """Every event body and every ITX body of `c`, ITX form and fields form,
    from each shard's slices and bases alone; returns the shards' bases."""
    fb, xb = c.packed, c.packed_frag
    all_bases = []
    for a, z, lo, hi in _shards(fb.ev.events, D):
        sl, bases = emu.slice_fields(fb, a, z, lo, hi)
        dig = emu.ev_body_hash(sl, bases, a, z)
        for e in range(a, z):
            assert dig[e - a].tobytes() == hashlib.sha256(c.raw[e]).digest(), ("fields", e)
        slx, bx = emu.slice_itx(xb, a, z, lo, hi)
        dig = emu.ev_body_hash(slx, bx, a, z)
        for e in range(a, z):
            assert dig[e - a].tobytes() == hashlib.sha256(c.raw[e]).digest(), ("itx", e)
        if fb.ev.itx_start is not None:
            i0 = int(fb.ev.itx_start[a])
            for form, (s, b) in (("fields", (sl.ev, bases)), ("itx", (slx, bx))):
                idig = emu.itx_body_hash(s, b)
                assert len(idig) == int(fb.ev.itx_start[z]) - i0
                for i in range(len(idig)):
                    assert idig[i].tobytes() == hashlib.sha256(c.itx_raw[i0 + i]).digest(), (form, i0 + i)
        all_bases.append((bases, bx))
    return all_bases


def test_rebased_serialisers_every_base():
    c = _case200()
    fb = c.packed
    assert [s[:2] for s in _shards(fb.ev.events, 4)] == [(0, 64), (64, 128), (128, 192), (192, 200)]
    all_bases = _check_bodies(c, 4)
    assert sum(len(b.InternalTransactions or []) for b in c.bodies) == len(c.itx_raw) > 100
    # in some shard >= 1 every base is non-zero (the block-signature fragments' for the ITX form)
    assert any(all(fbases[k] > 0 for k in ("ev", "tx", "txb", "ph", "itx", "str", "bsig", "sig", "val"))
               for fbases, _ in all_bases[1:]), [b for b, _ in all_bases]
    assert any(all(xbases[k] > 0 for k in ("ev", "tx", "txb", "ph", "itx", "str", "frag_bsig"))
               for _, xbases in all_bases[1:])
    # the validator bytes are read through their base: a BSIG_VAL_BYTES entry past shard 0
    assert fb.bsig_val_kind is not None and (fb.bsig_val_kind[int(fb.bsig_start[64]):] == E.BSIG_VAL_BYTES).any()
    assert all_bases[0][0] == dict.fromkeys(emu.BASES, 0)


def test_rebased_serialisers_shard_without_itx_or_bsig():
    specs = cycle_specs(192)
    for s in specs[64:128]:
        s["itxs"], s["bsigs"] = None, None
    c = FieldsCase(specs)
    fb = c.packed
    assert fb.ev.itx_start[64] == fb.ev.itx_start[128] > 0 and fb.bsig_start[64] == fb.bsig_start[128] > 0
    assert fb.ev.itx_start[192] > fb.ev.itx_start[128] and fb.bsig_start[192] > fb.bsig_start[128]
    _check_bodies(c, 3)


def test_rebased_serialisers_no_itx_fields():
    c = FieldsCase(cycle_specs(200, itxs=False), itx_fields=False)
    assert c.packed.ev.itx_start is None and c.packed.ev.itx_list_nil is not None
    bases = _check_bodies(c, 4)
    assert all(b["itx"] == 0 and b["str"] == 0 for b, _ in bases) and bases[2][0]["bsig"] > 0


def test_rebased_fold_per_shard():
    c = _case200()
    st, by, ist, bits = c.expected()
    assert {0, 1, 4} <= set(st.tolist()) and (by != E.EV_SELF).any()
    xb = c.packed.ev
    own, force = [], []  # the items as the verify kernels leave them: each signature's own class
    for body, sig in zip(c.bodies, c.signatures):
        own.append(G.item_status_from_sigstr(body.Creator, body.Hash(), sig))
    for t in c.itxs:
        force.append(len(E._go_bytes(t.Body.Peer.PubKeyHex)) < 2)
    own, force = np.array(own, np.uint8), np.array(force, np.uint8)
    # an ITX's item is its signature's own class; where force is set the fold must not read it: ACCEPT there
    assert force.sum() == 3 and (ist[force == 1] == 3).all()
    itx_items = np.where(force == 1, 1, ist).astype(np.uint8)
    for a, z, _, _ in _shards(xb.events, 4):
        i0, i1 = int(xb.itx_start[a]), int(xb.itx_start[z])
        items = np.concatenate([own[a:z], itx_items[i0:i1]])
        assert a == 0 or force[i0:i1].any()
        s_st, s_by, s_bits, s_ist = emu.compose(xb.itx_start[a:z + 1], i0, items, force[i0:i1])
        assert np.array_equal(s_st, st[a:z]) and np.array_equal(s_by, by[a:z]) and np.array_equal(s_ist, ist[i0:i1])
        # the shard's words are the matching words of the whole batch's mask (64-aligned shards)
        assert a % 64 == 0 and np.array_equal(s_bits, bits[a // 64:(z + 63) // 64])
        if a:
            assert i0 > 0
    # a forced panic wins over whatever the item says
    s_st, s_by, _, s_ist = emu.compose(np.array([5, 6, 7], np.uint64), 5, np.array([1, 1, 1, 1], np.uint8), [0, 1])
    assert s_st.tolist() == [1, 3] and s_by.tolist() == [E.EV_SELF, 0] and s_ist.tolist() == [1, 3]


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def test_new_symbols_resolve_and_reject_null():
    L = native.lib()
    for name in ("bv_group_verify_events_itx", "bv_group_verify_events_fields", "bv_plan_event_fields_shards"):
        assert name in native.EXPORTS and getattr(L, name) is not None
    assert L.bv_abi_version() == 6
    x, f, r = E.BvEventItxBatch(), E.BvEventFieldsBatch(), native.BvResult()
    assert L.bv_group_verify_events_itx(None, None, None, None) == native.BV_E_ARGS
    assert L.bv_group_verify_events_itx(None, ctypes.addressof(x), ctypes.byref(r), None) == native.BV_E_ARGS
    assert L.bv_group_verify_events_fields(None, None, None, None) == native.BV_E_ARGS
    assert L.bv_group_verify_events_fields(None, ctypes.addressof(f), ctypes.byref(r), None) == native.BV_E_ARGS
    import babble_amd

    assert babble_amd.Group.verify_events_itx and babble_amd.Group.verify_events_fields
    assert babble_amd.Group.verify_events_itx_into and babble_amd.Group.verify_events_fields_into
    assert babble_amd.plan_event_fields_shards is plan_event_fields_shards
