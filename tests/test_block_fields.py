"""bv_verify_blocks without a device: the BlockBody serialiser
(babble_amd/csrc/blkjson.h) through its public host form (bv_block_body_lens,
bv_block_bodies) and through the device's streaming SHA sink built for the host
(tests/emu_blocks), the argument checks, and the Python mirror's block paths
over a stub verifier.

Judge of every byte: oracle/gosemantics.py BlockBody.Marshal(); of every
digest: hashlib.sha256 over those bytes.  The grid is tests/block_cases.py
grid_bodies(): the full product of 7 hash options x 8 Transactions options x 4
fragment options x 4 integer options in which each of the three hashes takes
each of {nil, empty, 1, 2, 3, 32, 33 bytes}; all 7^3 hash combinations are
added on their own."""
import ctypes
import hashlib
import subprocess

import numpy as np
import pytest

from babble_amd import hashgraph as H
from babble_amd import native
from babble_amd.batch import BlockBatchBuilder
from oracle import gosemantics as G
from tests import block_cases as BC
from tests.emu_blocks import emu_blocks

_packed = {}


def packed(name):
    """(bodies, PackedBlockBatch) of a named body list, built once."""
    if name not in _packed:
        bodies = {"grid": BC.grid_bodies, "hashes": BC.hash_product_bodies,
                  "random": lambda: BC.random_bodies(2000, seed=20),
                  "pad": lambda: [BC.padded_body(t, 128) for t in (55, 56, 63, 64, 119, 120)]}[name]()
        kb = BlockBatchBuilder()
        for b in bodies:
            kb.add_block(b)
        _packed[name] = (bodies, kb.pack())
    return _packed[name]


def test_grid_covers_every_option():
    bodies, _ = packed("grid")
    assert len(bodies) == 7 * 8 * 4 * 4
    for f in ("StateHash", "FrameHash", "PeersHash"):
        assert {getattr(b, f) for b in bodies} == set(BC.HASHES) and len(BC.HASHES) == 7
        assert sorted(len(h) for h in BC.HASHES if h is not None) == [0, 1, 2, 3, 32, 33]
    for f in ("Index", "RoundReceived", "Timestamp"):
        assert {getattr(b, f) for b in bodies} == {0, -1, 2**63 - 1, -2**63}
    txs = {None if b.Transactions is None else tuple(b.Transactions) for b in bodies}
    assert txs == {None, (), (None,), (b"",), (b"a",), (b"ab",), (b"abc",), (bytes(range(64)),)}
    frags = {(G.json_list(b.InternalTransactions, lambda t: t.json()),
              G.json_list(b.InternalTransactionReceipts, lambda t: t.json())) for b in bodies}
    assert len(frags) == 4 and (b"null", b"null") in frags and (b"[]", b"[]") in frags
    assert any(i.startswith(b'[{"Body"') for i, _ in frags) and any(r.startswith(b'[{"Internal') for _, r in frags)


@pytest.mark.parametrize("name", ["grid", "hashes", "random"])
def test_block_bodies_equal_the_oracle_byte_for_byte(name):
    bodies, pb = packed(name)
    want = [b.Marshal() for b in bodies]
    off = pb.body_lens()
    assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), [len(w) for w in want])
    buf, off2 = pb.bodies()
    assert np.array_equal(off, off2)
    got = buf.tobytes()
    assert got == b"".join(want), next(i for i, w in enumerate(want) if got[int(off[i]):int(off[i + 1])] != w)


def test_block_bodies_at_caller_offsets():
    """bv_block_bodies writes each body at the caller's offset and nothing else."""
    bodies, pb = packed("hashes")
    lens = np.diff(pb.body_lens().astype(np.int64))
    off = np.zeros(len(bodies) + 1, np.uint64)
    off[1:] = np.cumsum(lens + 3)  # 3 spare bytes after every body
    out = np.full(int(off[-1]), 0xEE, np.uint8)
    keep = []
    cb = pb.c_struct(keep)
    assert native.lib().bv_block_bodies(cb, off.ctypes.data, out.ctypes.data) == native.BV_OK
    for i, b in enumerate(bodies):
        a = int(off[i])
        assert out[a:a + lens[i]].tobytes() == b.Marshal() and out[a + lens[i]:a + lens[i] + 3].tolist() == [0xEE] * 3


@pytest.mark.parametrize("name", ["grid", "hashes", "random", "pad"])
def test_streaming_sha_sink_equals_hashlib(name):
    """blk_emit into the EvjSha sink (the device's path, built for the host):
    every digest equals hashlib.sha256 of the oracle's bytes."""
    bodies, pb = packed(name)
    want = np.frombuffer(b"".join(hashlib.sha256(b.Marshal()).digest() for b in bodies), np.uint8).reshape(-1, 32)
    assert np.array_equal(emu_blocks.body_len(pb), [len(b.Marshal()) for b in bodies])
    got = emu_blocks.body_hash(pb)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]


def test_padding_boundary_bodies_have_the_lengths():
    """One transaction pads the body to 55, 56, 63, 64, 119 and 120 bytes
    modulo 128: the last SHA block holds 55 bytes (the length still fits), 56
    (it no longer does: one more block), 63 and 64 / 0 (a full block), on an
    odd and on an even number of blocks."""
    bodies, _ = packed("pad")
    assert [len(b.Marshal()) % 128 for b in bodies] == [55, 56, 63, 64, 119, 120]
    assert [len(b.Marshal()) % 64 for b in bodies] == [55, 56, 63, 0, 55, 56]
    assert all(len(b.Transactions) == 1 for b in bodies)


def test_null_and_bad_arguments_without_a_device():
    L = native.lib()
    assert L.bv_verify_blocks(None, None, None, None) == native.BV_E_ARGS
    bodies, pb = packed("hashes")
    keep = []
    cb = pb.c_struct(keep)
    r = native.BvResult()
    assert L.bv_verify_blocks(None, ctypes.byref(cb), ctypes.byref(r), None) == native.BV_E_ARGS
    off = pb.body_lens()
    out = np.zeros(int(off[-1]), np.uint8)
    assert L.bv_block_body_lens(None, off.ctypes.data) == native.BV_E_ARGS
    assert L.bv_block_body_lens(cb, None) == native.BV_E_ARGS
    assert L.bv_block_bodies(None, off.ctypes.data, out.ctypes.data) == native.BV_E_ARGS
    assert L.bv_block_bodies(cb, None, out.ctypes.data) == native.BV_E_ARGS
    assert L.bv_block_bodies(cb, off.ctypes.data, None) == native.BV_E_ARGS
    # a slot shorter than its body, offsets going down
    short = off.copy()
    short[1:] -= 1
    assert L.bv_block_bodies(cb, short.ctypes.data, out.ctypes.data) == native.BV_E_ARGS
    down = off.copy()
    down[3] = down[2] - 1
    assert L.bv_block_bodies(cb, down.ctypes.data, out.ctypes.data) == native.BV_E_ARGS

    def broken(name, edit):
        a = np.array(getattr(pb, name), copy=True)
        edit(a)
        k2 = []
        c2 = pb.c_struct(k2)
        k2.append(a)
        setattr(c2, name, a.ctypes.data)
        return c2, k2

    def not_from_zero(a):
        a[0] = 1

    def goes_down(a):
        a[len(a) // 2] = a[len(a) // 2 + 1] + 1

    for name in ("hash_off", "tx_start", "tx_off"):
        for edit in (not_from_zero, goes_down):
            c2, k2 = broken(name, edit)
            assert L.bv_block_body_lens(c2, off.ctypes.data) == native.BV_E_ARGS, (name, edit.__name__)
            assert L.bv_block_bodies(c2, off.ctypes.data, out.ctypes.data) == native.BV_E_ARGS, (name, edit.__name__)
    for name in ("index", "round_received", "timestamp", "hash_off", "hash_bytes", "tx_start", "tx_off", "tx_bytes"):
        c2 = pb.c_struct(keep)
        setattr(c2, name, None)
        assert L.bv_block_body_lens(c2, off.ctypes.data) == native.BV_E_ARGS, name
    # fragments: offsets from 0, monotone, bytes present
    _, gp = packed("grid")
    c3, k3 = None, []
    for name in ("itx_off", "rcpt_off"):
        goff = np.zeros(gp.n_blocks + 1, np.uint64)
        for edit in (not_from_zero, goes_down):
            a = np.array(getattr(gp, name), copy=True)
            edit(a)
            c3 = gp.c_struct(k3)
            k3.append(a)
            setattr(c3, name, a.ctypes.data)
            assert L.bv_block_body_lens(c3, goff.ctypes.data) == native.BV_E_ARGS, (name, edit.__name__)
    c3 = gp.c_struct(k3)
    c3.itx_json = None
    assert L.bv_block_body_lens(c3, np.zeros(gp.n_blocks + 1, np.uint64).ctypes.data) == native.BV_E_ARGS
    # more than 2^32 blocks: refused before any array is read
    c4 = pb.c_struct(keep)
    c4.n_blocks = 2**32 + 1
    assert L.bv_block_body_lens(c4, off.ctypes.data) == native.BV_E_ARGS
    # no blocks: BV_OK, one offset written, nothing else touched
    empty = BlockBatchBuilder().pack()
    ce = empty.c_struct(keep)
    o1 = np.full(1, 7, np.uint64)
    assert L.bv_block_body_lens(ce, o1.ctypes.data) == native.BV_OK and o1[0] == 0
    assert L.bv_block_bodies(ce, o1.ctypes.data, None) == native.BV_OK
    assert empty.bodies()[0].size == 0


# ----------------------------------------------------------------------------
# the mirror over a stub verifier
# ----------------------------------------------------------------------------
class StubVerifier:
    """Decides every item from its signature text alone: r == 1 ACCEPT, any
    other parsed r REJECT, wrong part count REJECT_ERR, an unparsable r
    REF_PANIC (the statuses are then the same whichever entry carries the
    item); records what each entry was given."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _status(pre, r_be):
        st = np.zeros(len(pre), np.uint8)
        for i in range(len(pre)):
            if pre[i] & native.PRE_PARTS_BAD:
                st[i] = native.REJECT_ERR
            elif (pre[i] & 3) == native.SC_NIL:
                st[i] = native.REF_PANIC
            else:
                st[i] = native.ACCEPT if int.from_bytes(r_be[i].tobytes(), "big") == 1 else native.REJECT
        return st

    def _result(self, st, n_msgs, item_msg, counts):
        from babble_amd.verifier import BlockVerifyResult

        bits = np.packbits(st == 1, bitorder="little")
        bits = np.concatenate([bits, np.zeros((-len(bits)) % 8, np.uint8)]).view(np.uint64)
        vc = np.bincount(item_msg[st == 1], minlength=n_msgs).astype(np.uint32) if counts else None
        return BlockVerifyResult(np.zeros((n_msgs, 32), np.uint8), st, bits, vc)

    def verify(self, b):
        self.calls.append(("verify", b.n_msgs, b.n_items, [b.message(m) for m in range(b.n_msgs)]))
        return self._result(self._status(b.pre, b.r_be), b.n_msgs, b.item_msg, False)

    def verify_text(self, tb):
        d = tb.decoded()
        self.calls.append(("verify_text", d.n_msgs, d.n_items, [d.message(m) for m in range(d.n_msgs)]))
        return self._result(self._status(d.pre, d.r_be), d.n_msgs, d.item_msg, False)

    def verify_blocks(self, pb, counts=True, status=True):
        d = pb.decoded()
        buf, off = pb.bodies()
        self.calls.append(("verify_blocks", pb.n_blocks, pb.n_items,
                           [buf[int(off[m]):int(off[m + 1])].tobytes() for m in range(pb.n_blocks)]))
        return self._result(self._status(d.pre, d.r_be), pb.n_blocks, pb.item_block, counts)

    def peer_set_hash(self, pks):
        h = b""
        for pk in pks:
            h = hashlib.sha256(h + pk).digest()
        return h


def _peer_set(n):
    return H.PeerSet([H.Peer(PubKeyHex=H.EncodeToString(pub)) for _, pub in BC.validators(n)])


def _block(index, ps_hash, sig_texts, n_validators, itx=None):
    body = H.BlockBody(Index=index, RoundReceived=index + 1, Timestamp=1_600_000_000 + index, StateHash=b"s" * 32,
                       FrameHash=None, PeersHash=ps_hash, Transactions=[b"tx%d" % index, None, b""],
                       InternalTransactions=itx, InternalTransactionReceipts=[])
    blk = H.Block(Body=body)
    for (_, pub), text in zip(BC.validators(n_validators), sig_texts):
        blk.Signatures[H.EncodeToString(pub)] = text
    return blk


def test_check_blocks_returns_what_check_block_returns():
    v = StubVerifier()
    ps = _peer_set(4)  # TrustCount 2: more than 2 valid signatures pass
    small = _peer_set(2)
    good, bad = "1|5", "2|5"
    itx = [H.InternalTransaction(H.InternalTransactionBody(1, H.Peer("a", "0X04", "m")), "s|t")]
    blocks = [
        _block(0, ps.Hash(v), [good, good, good, bad], 4),
        _block(1, ps.Hash(v), [good, good, bad, bad], 4),           # 2 valid: not enough
        _block(2, b"\x00" * 32, [good] * 4, 4),                     # wrong PeerSet
        _block(3, None, [good] * 4, 4),                             # nil PeersHash never matches
        _block(4, ps.Hash(v), [good, good, good, "|5"], 4),         # an item where Go panics
        _block(5, ps.Hash(v), [good, "one part", good, good], 4),   # DecodeSignature's error: (false, err), not valid
        _block(6, small.Hash(v), [good, good, good, good], 4, itx),  # two signers outside its peer set: skipped
        _block(7, ps.Hash(v), [], 4),
    ]
    sets = [ps, ps, ps, ps, ps, ps, small, ps]
    want = []
    for blk, s in zip(blocks, sets):
        try:
            want.append(H.check_block(blk, s, v))
        except native.ReferencePanic as e:
            want.append(("panic", str(e)))
    v.calls.clear()
    got = H.check_blocks(blocks, sets, v)
    got = [("panic", str(g)) if isinstance(g, native.ReferencePanic) else g for g in got]
    assert got == want
    assert want == [None, "Not enough valid signatures: got 2, need 2", "Wrong PeerSet", "Wrong PeerSet",
                    ("panic", "Block.Verify panics"), None, None, "Not enough valid signatures: got 0, need 2"]
    # ONE call: the six blocks whose PeerSet matched, their listed signatures only, the bodies from the fields
    assert len(v.calls) == 1
    name, n_blocks, n_items, bodies = v.calls[0]
    assert (name, n_blocks, n_items) == ("verify_blocks", 6, 4 * 4 + 2 + 0)
    assert bodies == [blocks[i].Body.Marshal() for i in (0, 1, 4, 5, 6, 7)]
    assert H.check_blocks([], [], v) == [] and H.check_blocks(blocks[2:4], sets[2:4], v) == ["Wrong PeerSet"] * 2


def test_fields_entries_equal_the_serialised_ones():
    v = StubVerifier()
    ps = _peer_set(5)
    texts = ["1|5", "2|5", "|5", "a|b|c", "1|1"]
    blk = _block(9, ps.Hash(v), texts, 5)
    sigs = blk.GetSignatures()
    a = H.verify_block_signatures(blk, sigs, v)
    b = H.verify_block_signatures(blk, sigs, v, text=True)
    c = H.verify_block_signatures(blk, sigs, v, fields=True)
    assert a == b == c and [o.ok for o in c] == [True, False, False, False, True]
    assert c[2].panic and c[3].err == "wrong number of values in signature: got 3, want 2"
    assert [x[0] for x in v.calls] == ["verify", "verify_text", "verify_blocks"]
    assert v.calls[0][3] == v.calls[1][3] == v.calls[2][3] == [blk.Body.Marshal()]
    assert H.verify_block_signatures(blk, [], v, fields=True) == []
    # ProcessSigPool: two blocks, a rejected signature skipped, the pool aborted at DecodeSignature's error
    outs = []
    for kw in ({}, {"text": True}, {"fields": True}):
        b1, b2 = _block(1, ps.Hash(v), [], 5), _block(2, ps.Hash(v), [], 5)
        pubs = [pub for _, pub in BC.validators(5)]
        pending = [H.BlockSignature(pubs[0], 1, "1|5"), H.BlockSignature(pubs[1], 2, "1|7"),
                   H.BlockSignature(pubs[2], 1, "2|5"), H.BlockSignature(b"\x04" * 65, 1, "1|5"),  # not a peer
                   H.BlockSignature(pubs[3], 3, "1|5"),  # no such block
                   H.BlockSignature(pubs[3], 2, "1|9"), H.BlockSignature(pubs[4], 1, "one part"),
                   H.BlockSignature(pubs[4], 2, "1|5")]
        v.calls.clear()
        appended, err = H.process_sig_pool(pending, lambda i: {1: b1, 2: b2}.get(i), lambda r: ps, v, **kw)
        outs.append(([(s.Index, s.Signature) for s in appended], err, dict(b1.Signatures), dict(b2.Signatures),
                     v.calls[0][1:3], sorted(v.calls[0][3])))
    assert outs[0] == outs[1] == outs[2]
    assert outs[2][0] == [(1, "1|5"), (2, "1|7"), (2, "1|9")] and outs[2][1].startswith("wrong number of values")
    assert outs[2][4] == (2, 6)


def test_serialiser_fuzz_under_asan_ubsan():
    """The stand-alone fuzz driver (its own main; ASan + UBSan; host code
    only): random batches in exactly-sized arrays, blk_len against what
    blk_emit writes, the SHA sink's byte count."""
    exe = emu_blocks.fuzz_exe()
    for seed in (1, 2, 3):
        p = subprocess.run([exe, str(seed), "150"], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.startswith("ok "), (seed, p.stdout[-500:], p.stderr[-2000:])
        assert int(p.stdout.split()[1]) > 300
