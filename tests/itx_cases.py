"""Shared cases of the bv_verify_events_itx tests (tests/test_event_itx.py on
the CPU, tests/test_gpu_event_itx.py on the device): events that carry
InternalTransactions, signed with the project's generator
(tests/block_cases.py), the packed field batch and what the oracle
(oracle/gosemantics.py) says about every event and every ITX.  Not a test
module.
"""
from __future__ import annotations

import hashlib
import random
from typing import List, Optional, Sequence

import numpy as np

from babble_amd import events as E
from oracle import gosemantics as G
from tests.block_cases import sign, validators

EV_SELF = 0xFFFFFFFF


def pub_hex(pub: bytes) -> str:
    return "0X" + pub.hex().upper()


def corrupt(text: str) -> str:
    """Another s (one digit changed): a well-formed signature that is REJECT."""
    return text[:-1] + ("1" if text[-1] != "1" else "2")


def make_itx(v: int, typ: int = 0, netaddr="node:1337", moniker="m", good: bool = True, pubhex=None,
             signature=None) -> G.InternalTransaction:
    """An ITX about validator v's peer, signed by v (or with `signature`)."""
    d, pub = validators(v + 1)[v]
    body = G.InternalTransactionBody(typ, G.Peer(netaddr, pub_hex(pub) if pubhex is None else pubhex, moniker))
    if signature is None:
        signature = sign(d, hashlib.sha256(body.Marshal()).digest(), typ)
        if not good:
            signature = corrupt(signature)
    return G.InternalTransaction(body, signature)


class ItxCase:
    """Events given as dicts (creator validator index `c`, `index`, `ts`,
    `parents` as EventBatchBuilder takes them, `txs`, `itxs` = None / list of
    G.InternalTransaction, `good` = sign the event validly, or `signature`).
    Builds the oracle bodies (in-batch parents resolved in order), the
    signatures, the packed batch and the expected results."""

    def __init__(self, specs: Sequence[dict], n_validators: int = 4):
        vs = validators(n_validators)
        b = E.EventBatchBuilder()
        kidx = [b.add_key(pub) for _, pub in vs]
        self.bodies: List[G.EventBody] = []
        self.signatures: List[str] = []
        self.raw: List[bytes] = []
        digests: List[bytes] = []
        for s in specs:
            pstr = []
            for p in s.get("parents", [None, None]):
                pstr.append("" if p is None else G.EncodeToString(p[1] if p[0] == "hash" else digests[p[1]]))
            body = G.EventBody(Transactions=s.get("txs"), InternalTransactions=s.get("itxs"), Parents=pstr,
                               Creator=vs[s["c"]][1], Index=s.get("index", 0), BlockSignatures=None,
                               Timestamp=s.get("ts", 0))
            raw = body.Marshal()
            dig = hashlib.sha256(raw).digest()
            sig = s.get("signature")
            if sig is None:
                sig = sign(vs[s["c"]][0], dig, len(digests))
                if not s.get("good", True):
                    sig = corrupt(sig)
            b.add_event(kidx[s["c"]], body.Index, body.Timestamp, s.get("parents", [None, None]), s.get("txs"), sig,
                        itxs=s.get("itxs"))
            self.bodies.append(body)
            self.signatures.append(sig)
            self.raw.append(raw)
            digests.append(dig)
        self.packed = b.pack_itx()
        self.digests = np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32)
        self.itxs = [t for body in self.bodies for t in (body.InternalTransactions or [])]
        self.itx_raw = [t.Body.Marshal() for t in self.itxs]
        self.itx_digests = np.frombuffer(b"".join(hashlib.sha256(r).digest() for r in self.itx_raw),
                                         np.uint8).reshape(-1, 32)
        self._expected = None

    @property
    def n(self) -> int:
        return len(self.bodies)

    def expected(self):
        """(event status [n], decided_by [n], itx status [n_itx], bitmask words)
        from the oracle, computed once."""
        if self._expected is None:
            st, by, ist = [], [], []
            for body, sig in zip(self.bodies, self.signatures):
                own = [G.itx_status(t) for t in (body.InternalTransactions or [])]
                ist += own
                first = next((j for j, c in enumerate(own) if c != G.ACCEPT), None)
                by.append(EV_SELF if first is None else first)
                st.append(G.event_status(body, sig))
            st = np.array(st, np.uint8)
            bits = np.zeros((len(st) + 63) // 64, np.uint64)
            for e in np.flatnonzero(st == 1):
                bits[e // 64] |= np.uint64(1) << np.uint64(e % 64)
            self._expected = (st, np.array(by, np.uint32), np.array(ist, np.uint8), bits)
        return self._expected


def cycle_specs(n: int, seed: int = 3, bad_every: int = 5) -> List[dict]:
    """n bulk events (parents by hash or none) whose ITX lists cycle nil / [] /
    1 / 2 / 3 ITXs; every bad_every-th signature (event or ITX) is corrupted."""
    rng = random.Random(seed)
    specs, k = [], 0
    for e in range(n):
        shape = e % 5
        itxs: Optional[list] = None if shape == 0 else []
        for j in range(max(shape - 1, 0)):
            k += 1
            itxs.append(make_itx((e + j) % 4, typ=j % 2, netaddr="n%d:%d" % (e, j), moniker="mon<%d>" % k,
                                 good=k % bad_every != 0))
        par = [None if e % 3 == 0 else ("hash", bytes(rng.getrandbits(8) for _ in range(32))),
               None if e % 4 == 0 else ("hash", bytes(rng.getrandbits(8) for _ in range(32)))]
        txs = None if e % 7 == 0 else [bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 40)))
                                       for _ in range(e % 3)]
        specs.append(dict(c=e % 4, index=e, ts=1600000000 + e, parents=par, txs=txs, itxs=itxs,
                          good=(e % bad_every) != 2))
    return specs


def string_grid() -> List[bytes]:
    """The strings of the escaping tests: empty, every single byte, lead x
    trail pairs, the named runes, sequences cut short, the HTML set, and 2,000
    seeded random byte strings of 0-40 bytes."""
    g = [b""] + [bytes([c]) for c in range(256)]
    g += pair_strings()
    g += [b"\xe2\x80\xa8", b"\xe2\x80\xa9", b"\xe2\x80\xa7", b"\xef\xbf\xbd", b"\xf4\x8f\xbf\xbf",  # U+2028 U+2029 U+2027 U+FFFD U+10FFFF
          b"\xed\x9f\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xe2\x80", b"\xe2", b"\xf0\x9f\x98", b"\xf0\x9f",  # U+D7FF, surrogates, cut short
          b"\xf0", b"a\xe2\x80", b"a\xf0\x9f\x98", b"<>&\"\\"]
    rng = random.Random(2028)
    g += [bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 41))) for _ in range(2000)]
    return g


def pair_strings() -> List[bytes]:
    return [bytes([a, t]) for a in (0xC1, 0xC2, 0xDF, 0xE0, 0xED, 0xEF, 0xF0, 0xF4, 0xF5)
            for t in (0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0)]


def string_itx(s: bytes, pos: int) -> G.InternalTransaction:
    """An ITX with `s` in string position pos (0 NetAddr, 1 PubKeyHex, 2
    Moniker, 3 Signature), plain text elsewhere."""
    f = [b"addr", b"0X04", b"mon", b"1|2"]
    f[pos] = s
    return G.InternalTransaction(G.InternalTransactionBody(pos, G.Peer(f[0], f[1], f[2])), f[3])
