"""bv_group_verify_events' host side, CPU only: the event-shard plan
(bv_plan_event_shards, csrc/hostplan.cpp) against its Python restatement
(babble_amd/shard.py plan_event_shards) and its own properties, the same
cases through an ASan + UBSan build of hostplan.cpp (tests/hostfuzz_events, a
stand-alone driver run as a subprocess), and the rebased serialiser (evjson.h
evj_emit with EvjBases: what k_ev_body_hash_rb runs per lane) on the host,
given only a shard's slices and bases (tests/emu_shards), against hashlib over
the oracle's bodies."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from babble_amd import events as E
from babble_amd import native, shard, synth
from babble_amd.verifier import plan_event_shards
from tests.emu_shards import emu_shards
from tests.test_events import random_wire

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostfuzz_events")
EXE = os.path.join(HERE, "_build", "hostfuzz_events")


def _cases():
    """1,000 random (D, n_parent_hashes, kinds[n, 2], refs[n, 2]): n in
    [0, 700], D in [1, 9], 0..50 parent hashes; every second case gets at
    least one in-batch (EVENT) parent when it has two events."""
    rng = np.random.default_rng(41)
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
        out.append((D, nh, kinds, refs))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _c_plan(D, nh, kinds, refs):
    kinds = np.ascontiguousarray(kinds, np.uint8)
    refs = np.ascontiguousarray(refs, np.uint64)
    b = E.BvEventBatch()
    b.n_events = len(kinds)
    b.n_parent_hashes = nh
    # (never NULL: an empty batch still passes valid pointers)
    b.parent_kind = kinds.ctypes.data if kinds.size else np.zeros(1, np.uint8).ctypes.data
    b.parent_ref = refs.ctypes.data if refs.size else np.zeros(1, np.uint64).ctypes.data
    bounds = np.zeros(D + 1, np.uint64)
    lo = np.zeros(D, np.uint64)
    hi = np.zeros(D, np.uint64)
    rc = native.lib().bv_plan_event_shards(ctypes.addressof(b), D, bounds.ctypes.data, lo.ctypes.data,
                                           hi.ctypes.data)
    return rc, bounds.tolist(), lo.tolist(), hi.tolist()


def _check_properties(rc, bounds, lo, hi, D, kinds, refs):
    n = len(kinds)
    dag = bool(np.any(kinds == E.PARENT_EVENT))
    assert rc == (1 if dag else 0)
    assert bounds[0] == 0 and bounds[-1] == n and all(a <= b for a, b in zip(bounds, bounds[1:]))
    if dag:
        assert bounds == [0] + [n] * D
    else:
        # whole 64-event words, except where the last non-empty shard ends
        assert all(b % 64 == 0 or b == n for b in bounds)
        assert bounds == [shard.shard_bounds(n, D, d)[0] for d in range(D)] + [n]
    for d in range(D):
        r = refs[bounds[d]:bounds[d + 1]][kinds[bounds[d]:bounds[d + 1]] == E.PARENT_HASH]
        if r.size == 0:
            assert lo[d] == hi[d] == 0
        else:
            assert np.all((r >= lo[d]) & (r < hi[d]))
            assert lo[d] in r and hi[d] - 1 in r  # tight: both ends are referenced


def test_plan_c_equals_model_and_properties(cases):
    n_dag = 0
    for D, nh, kinds, refs in cases:
        rc, bounds, lo, hi = _c_plan(D, nh, kinds, refs)
        dag, mb, mlo, mhi = shard.plan_event_shards(kinds, refs, D)
        assert rc == int(dag) and bounds == mb and lo == mlo and hi == mhi
        _check_properties(rc, bounds, lo, hi, D, kinds, refs)
        n_dag += rc
    assert 400 < n_dag < 600  # half bulk, half with an EVENT parent


def test_plan_fixed_cases():
    def plan(n, D):
        kinds = np.zeros((n, 2), np.uint8)
        return _c_plan(D, 0, kinds, np.zeros((n, 2), np.uint64))

    assert plan(100, 3) == (0, [0, 64, 100, 100], [0] * 3, [0] * 3)
    assert plan(130, 3) == (0, [0, 64, 128, 130], [0] * 3, [0] * 3)
    assert plan(0, 2) == (0, [0, 0, 0], [0] * 2, [0] * 2)
    assert plan(1, 8) == (0, [0] + [1] * 8, [0] * 8, [0] * 8)
    # hash ranges per shard, and a DAG batch whole on shard 0
    kinds = np.zeros((130, 2), np.uint8)
    refs = np.zeros((130, 2), np.uint64)
    for e, r in ((3, 7), (60, 2), (64, 9), (129, 40)):
        kinds[e, 1], refs[e, 1] = E.PARENT_HASH, r
    assert _c_plan(3, 41, kinds, refs) == (0, [0, 64, 128, 130], [2, 9, 40], [8, 10, 41])
    kinds[100, 0], refs[100, 0] = E.PARENT_EVENT, 99
    assert _c_plan(3, 41, kinds, refs) == (1, [0, 130, 130, 130], [2, 0, 0], [41, 0, 0])


def test_plan_bad_arguments():
    L = native.lib()
    kinds = np.array([[1, 0], [0, 1]], np.uint8)
    refs = np.array([[4, 0], [0, 5]], np.uint64)
    assert _c_plan(2, 6, kinds, refs)[0] == 0
    assert _c_plan(2, 5, kinds, refs)[0] == native.BV_E_ARGS  # a HASH ref >= n_parent_hashes
    assert _c_plan(2, 0, kinds, refs)[0] == native.BV_E_ARGS
    b = E.BvEventBatch()
    x = np.zeros(4, np.uint64)
    p = x.ctypes.data
    assert L.bv_plan_event_shards(None, 2, p, p, p) == native.BV_E_ARGS
    assert L.bv_plan_event_shards(ctypes.addressof(b), 2, None, p, p) == native.BV_E_ARGS
    assert L.bv_plan_event_shards(ctypes.addressof(b), 2, p, None, p) == native.BV_E_ARGS
    assert L.bv_plan_event_shards(ctypes.addressof(b), 2, p, p, None) == native.BV_E_ARGS
    assert L.bv_plan_event_shards(ctypes.addressof(b), 0, p, p, p) == native.BV_E_ARGS
    assert L.bv_plan_event_shards(ctypes.addressof(b), -3, p, p, p) == native.BV_E_ARGS


def test_plan_python_binding():
    _, wire = synth.event_fields(300, n_creators=5, seed=8, parents="hash")
    dag, bounds, lo, hi = plan_event_shards(wire, 3)
    want = shard.plan_event_shards(wire.parent_kind, wire.parent_ref, 3)
    assert (dag, bounds.tolist(), lo.tolist(), hi.tolist()) == want and not dag
    _, wire = synth.event_fields(50, n_creators=3, seed=8, parents="event")
    dag, bounds, lo, hi = plan_event_shards(wire, 2)
    assert dag and bounds.tolist() == [0, 50, 50]


def test_plan_fuzz_sanitized(cases):
    """The same random cases through hostplan.cpp built with ASan + UBSan, each
    copied into exactly-sized heap buffers by the stand-alone driver."""
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    lines = []
    for D, nh, kinds, refs in cases:
        ks = "".join(map(str, kinds.reshape(-1).tolist())) or "-"
        rs = ",".join(map(str, refs.reshape(-1).tolist())) or "-"
        lines.append(f"P {D} {len(kinds)} {nh} {ks} {rs}")
    lines += ["P 2 2 5 1001 4,0,0,5", "P 2 2 6 1001 4,0,0,5", "P 1 1 3 30 0,0", "N"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    for (D, nh, kinds, refs), line in zip(cases, out):
        f = line.split()
        dag, mb, mlo, mhi = shard.plan_event_shards(kinds, refs, D)
        assert f[0] == "P" and int(f[1]) == int(dag)
        assert [[int(x) for x in g.split(",")] for g in f[2:]] == [mb, mlo, mhi]
    assert out[-4] == "P -1"  # a HASH ref >= n_parent_hashes: refused
    assert out[-3] == "P 0 0,2,2 4,0 6,0"
    assert out[-2] == "P -1"  # an unknown parent kind
    assert out[-1] == "N -1 -1 -1 -1 -1"


# ---------------------------------------------------------------------------
# The rebased serialiser, given only a shard's slices and its bases
# ---------------------------------------------------------------------------
def _shard_digests(wire, D):
    """Every shard's digests from its slices alone, concatenated; also what
    the plan gave (for the coverage assertions)."""
    dag, bounds, lo, hi = shard.plan_event_shards(wire.parent_kind, wire.parent_ref, D)
    assert not dag
    out = []
    for d in range(D):
        a, z = bounds[d], bounds[d + 1]
        sl, bases = emu_shards.slice_wire(wire, a, z, lo[d], hi[d])
        assert sl.n_events == z - a and len(sl.parent_hashes) == hi[d] - lo[d]
        out.append(emu_shards.body_hash(sl, bases, a, z))
    return np.concatenate(out), bounds, lo, hi


@pytest.mark.parametrize("n", [500, 100, 1])
def test_rebased_serialiser_edge_bodies(n):
    """random_wire's edge bodies (nil and empty tx lists, nil txs, ITX and
    BlockSignature fragments, parents by hash) cut into 3 shards: each
    shard's digests, built from its slices and bases only, equal hashlib over
    the oracle's bodies of that event range; n = 100 and n = 1 leave empty
    shards."""
    for seed in (4, 5):
        wire, bodies, wd = random_wire(seed, n=n, in_batch=False)
        dig, bounds, lo, hi = _shard_digests(wire, 3)
        assert len(dig) == n
        for e in range(n):
            assert dig[e].tobytes() == hashlib.sha256(bodies[e]).digest(), (seed, e)
        if n == 500:  # what the cut goes through
            assert bounds == [0, 192, 384, 500] and all(l > 0 for l in lo[1:])
            assert wire.tx_list_nil is not None and wire.tx_nil is not None
            assert wire.itx_off is not None and int(wire.itx_off[bounds[1]]) > 0
            assert wire.bsig_off is not None and int(wire.bsig_off[bounds[1]]) > 0
            assert int(wire.tx_start[bounds[1]]) > 0 and int(wire.tx_off[int(wire.tx_start[bounds[1]])]) > 0
        else:
            assert bounds[-2] == bounds[-1]  # an empty shard


def test_rebased_serialiser_signed_events():
    packed, wire = synth.event_fields(300, n_creators=5, parents="hash")
    dig, bounds, lo, hi = _shard_digests(wire, 3)
    assert bounds == [0, 128, 256, 300]
    for e in range(300):
        assert dig[e].tobytes() == hashlib.sha256(packed.message(e)).digest(), e
    # parent hashes at both ends of each shard's range are read through the base
    for d in range(3):
        r = wire.parent_ref[bounds[d]:bounds[d + 1]][wire.parent_kind[bounds[d]:bounds[d + 1]] == E.PARENT_HASH]
        assert lo[d] in r and hi[d] - 1 in r
    assert lo[1] > 0 and lo[2] > 0


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def test_new_symbols_resolve_and_reject_null():
    L = native.lib()
    for name in ("bv_group_verify_events", "bv_group_kc_register", "bv_plan_event_shards"):
        assert name in native.EXPORTS and getattr(L, name) is not None
    assert L.bv_group_verify_events(None, None, None) == native.BV_E_ARGS
    b = E.BvEventBatch()
    r = native.BvResult()
    assert L.bv_group_verify_events(None, ctypes.addressof(b), ctypes.byref(r)) == native.BV_E_ARGS
    assert L.bv_group_kc_register(None, 0, None, None) == native.BV_E_ARGS
    import babble_amd

    assert babble_amd.Group.verify_events and babble_amd.plan_event_shards is plan_event_shards
