"""Shared cases of the bv_verify_events_fields tests (tests/test_event_fields.py
on the CPU, tests/test_gpu_event_fields.py on the device): events that carry
BlockSignatures (and InternalTransactions), signed with the project's
generator, the packed field batch, the same events with ORACLE-built
BlockSignatures fragments for the entries that take fragments, and what the
oracle (oracle/gosemantics.py) says about every event and every ITX.  Not a
test module.
"""
from __future__ import annotations

import hashlib
import random
from typing import List, Optional, Sequence

import numpy as np

from babble_amd import events as E
from oracle import gosemantics as G
from tests.block_cases import sign, validators
from tests.itx_cases import (EV_SELF, ItxCase, corrupt, cycle_specs as itx_cycle_specs, make_itx,  # noqa: F401
                             pair_strings, string_grid)

INDEXES = [0, -1, 2 ** 63 - 1, -2 ** 63, 7, 1234567890123]


def bsig_fragment(bsigs: Optional[Sequence[G.BlockSignature]]) -> bytes:
    """encoding/json of the slice as the fragment entries take it (b"" = nil)."""
    return b"" if bsigs is None else G.json_list(bsigs, lambda t: t.json())


class FieldsCase(ItxCase):
    """ItxCase's specs with `bsigs` = None / list of G.BlockSignature per event.
    packed: the bv_event_fields_batch (itx_fields: pack_fields' argument);
    packed_frag: the bv_event_itx_batch over the same events with the oracle's
    BlockSignatures fragments; expected() is ItxCase's (the block signatures
    change the bodies, not the rules)."""

    def __init__(self, specs: Sequence[dict], n_validators: int = 4, itx_fields: Optional[bool] = True):
        vs = validators(n_validators)
        b, bf = E.EventBatchBuilder(), E.EventBatchBuilder()
        kidx = [b.add_key(pub) for _, pub in vs]
        for _, pub in vs:
            bf.add_key(pub)
        self.bodies: List[G.EventBody] = []
        self.signatures: List[str] = []
        self.raw: List[bytes] = []
        digests: List[bytes] = []
        for s in specs:
            pstr = []
            for p in s.get("parents", [None, None]):
                pstr.append("" if p is None else G.EncodeToString(p[1] if p[0] == "hash" else digests[p[1]]))
            body = G.EventBody(Transactions=s.get("txs"), InternalTransactions=s.get("itxs"), Parents=pstr,
                               Creator=vs[s["c"]][1], Index=s.get("index", 0), BlockSignatures=s.get("bsigs"),
                               Timestamp=s.get("ts", 0))
            raw = body.Marshal()
            dig = hashlib.sha256(raw).digest()
            sig = s.get("signature")
            if sig is None:
                sig = sign(vs[s["c"]][0], dig, len(digests))
                if not s.get("good", True):
                    sig = corrupt(sig)
            args = (kidx[s["c"]], body.Index, body.Timestamp, s.get("parents", [None, None]), s.get("txs"), sig)
            b.add_event(*args, itxs=s.get("itxs"), bsigs=s.get("bsigs"))
            bf.add_event(*args, itxs=s.get("itxs"), bsig_json=bsig_fragment(s.get("bsigs")))
            self.bodies.append(body)
            self.signatures.append(sig)
            self.raw.append(raw)
            digests.append(dig)
        self.packed = b.pack_fields(itx_fields=itx_fields)
        self.packed_frag = bf.pack_itx()
        self.digests = np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32)
        self.itxs = [t for body in self.bodies for t in (body.InternalTransactions or [])]
        self.itx_raw = [t.Body.Marshal() for t in self.itxs]
        self.itx_digests = np.frombuffer(b"".join(hashlib.sha256(r).digest() for r in self.itx_raw),
                                         np.uint8).reshape(-1, 32)
        self._expected = None

    def events_frag(self) -> E.EventWireBatch:
        """packed_frag's events with the InternalTransactions as oracle-built
        fragments too: what bv_verify_events takes (it verifies no ITX)."""
        import dataclasses

        frags = [b"" if b.InternalTransactions is None else G.json_list(b.InternalTransactions, lambda t: t.json())
                 for b in self.bodies]
        off = np.zeros(self.n + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in frags], dtype=np.uint64)
        return dataclasses.replace(self.packed_frag.events, itx_off=off if any(frags) else None,
                                   itx_json=np.frombuffer(b"".join(frags), np.uint8).copy())


def block_sig(v: int, k: int, index: int, validator="creator", signature=None) -> G.BlockSignature:
    """Validator v's signature of 'block k': a real r|s text over a digest."""
    d, pub = validators(4)[v % 4]
    if signature is None:
        signature = sign(d, hashlib.sha256(b"block %d" % k).digest(), k)
    return G.BlockSignature(pub if validator == "creator" else validator, index, signature)


def add_cycle_bsigs(specs: List[dict]) -> List[dict]:
    """bsig lists nil / [] / 1 / 2 / 3 per event, shifted by one against the ITX
    lists of itx_cases.cycle_specs every 5 events (a period of 25 against 5:
    every combination occurs in 25 events); the Index values walk INDEXES; every 7th Validator is another
    validator's key (BV_BSIG_VAL_BYTES), every 11th nil."""
    k = 0
    for e, s in enumerate(specs):
        shape = (e + e // 5) % 5
        bsigs: Optional[list] = None if shape == 0 else []
        for j in range(max(shape - 1, 0)):
            val = "creator"
            if k % 7 == 3:
                val = validators(4)[(s["c"] + 1) % 4][1]
            elif k % 11 == 5:
                val = None
            bsigs.append(block_sig(s["c"], k, INDEXES[k % len(INDEXES)], val))
            k += 1
        s["bsigs"] = bsigs
    return specs


def cycle_specs(n: int, itxs: bool = True, **kw) -> List[dict]:
    specs = itx_cycle_specs(n, **kw)
    if not itxs:
        for e, s in enumerate(specs):
            s["itxs"] = None if e % 3 else []
    return add_cycle_bsigs(specs)


def signature_specs(strings: Sequence[bytes]) -> List[dict]:
    """One event per string: a single block signature with that Signature."""
    return [dict(c=e % 4, index=e, signature="1|2", bsigs=[block_sig(e % 4, e, e - 5, signature=s)])
            for e, s in enumerate(strings)]


def residue_specs() -> List[dict]:
    """A Signature of 0..130 bytes: body lengths cover every value mod 64."""
    return signature_specs([b"s" * k for k in range(131)])


def validator_specs() -> List[dict]:
    """Validator bytes of length 0, 1, 2, 3, 64, 65, 66 (every base64 tail),
    nil validators, nil against empty lists."""
    specs = []
    for e, ln in enumerate([0, 1, 2, 3, 64, 65, 66]):
        specs.append(dict(c=e % 4, index=e, signature="1|2",
                          bsigs=[block_sig(e, e, INDEXES[e % len(INDEXES)], bytes(range(1, ln + 1)))]))
    specs.append(dict(c=0, index=8, signature="1|2", bsigs=[block_sig(0, 1, 3, None), block_sig(0, 2, -4),
                                                            block_sig(1, 3, 5, b"")]))
    specs.append(dict(c=1, index=9, signature="1|2", bsigs=None))
    specs.append(dict(c=2, index=10, signature="1|2", bsigs=[]))
    specs.append(dict(c=3, index=11, signature="1|2", bsigs=None, itxs=[]))
    return specs


def dag_specs(n: int = 40, creators: int = 4, seed: int = 9) -> List[dict]:
    """A SyncResponse: each creator's events chain by self-parent, the other
    parent an earlier event of another creator (or a known hash for the first
    round); the events with in-batch parents carry block signatures, every
    fifth an ITX."""
    rng = random.Random(seed)
    last = {}
    specs, k = [], 0
    for e in range(n):
        c = e % creators
        sp = ("event", last[c]) if c in last else ("hash", bytes(rng.getrandbits(8) for _ in range(32)))
        others = [v for cc, v in last.items() if cc != c]
        op = ("event", rng.choice(others)) if others and e >= creators else None
        bsigs = None
        if sp[0] == "event" or (op and op[0] == "event"):
            bsigs = []
            for j in range(1 + e % 3):
                bsigs.append(block_sig(c, k, INDEXES[k % len(INDEXES)]))
                k += 1
        itxs = [make_itx((e + 1) % 4, netaddr="d%d" % e, good=e % 10 != 5)] if e % 5 == 0 else None
        specs.append(dict(c=c, index=e // creators, ts=1700000000 + e, parents=[sp, op],
                          txs=[bytes(rng.getrandbits(8) for _ in range(e % 50))], itxs=itxs, bsigs=bsigs,
                          good=e % 9 != 4))
        last[c] = e
    return specs
