"""Block workloads of tests/test_block_fields.py and
tests/test_gpu_block_fields.py: BlockBodies of the Go-semantics oracle
(oracle/gosemantics.py) with their canonical bytes, a validator set, and
block signatures over the oracle's digests.  Not a test module.

Signing is plain modular arithmetic: a signer draws its nonce k from a small
fixed pool, so r = x(k G) mod N and k^-1 are computed once per pool entry and
s = k^-1 (z + r d) mod N per signature (no scalar multiplication per item;
the oracle's pure-Python group law is only used for the pool and the keys).
"""
from __future__ import annotations

import hashlib
import random
from typing import List, Optional, Sequence

import numpy as np

from babble_amd.batch import BlockBatchBuilder, PackedBatch, PackedBlockBatch
from oracle import gosemantics as G

# the grid of the issue: every value of every dimension
HASHES = [None, b"", b"\x01", b"\x01\x02", b"\xff\x00\x7f", bytes(range(32)), bytes(range(200, 233))]
TXS = [None, [], [None], [b""], [b"a"], [b"ab"], [b"abc"], [bytes(range(64))]]
_PEER = G.Peer("node1:1337", "0X04AB", "monika")
_ITX = [G.InternalTransaction(G.InternalTransactionBody(0, _PEER), "1a|2b"),
        G.InternalTransaction(G.InternalTransactionBody(1, G.Peer()), "")]
_RCPT = [G.InternalTransactionReceipt(_ITX[0], True), G.InternalTransactionReceipt(_ITX[1], False)]
FRAGS = [(None, None), ([], []), (_ITX, None), (None, _RCPT)]  # (InternalTransactions, InternalTransactionReceipts)
INTS = [0, -1, 2**63 - 1, -2**63]


def grid_bodies() -> List[G.BlockBody]:
    """7 x 8 x 4 x 4 = 896 bodies: the full product of the hash, transaction,
    fragment and integer options.  Hash option h gives (StateHash, FrameHash,
    PeersHash) = (H[h], H[h+2], H[h+4]) (indices mod 7), so EACH of the three
    hashes takes every value of HASHES against every option of the other
    dimensions; integer option i gives (Index, RoundReceived, Timestamp) =
    (I[i], I[i+1], I[i+2]) (mod 4) likewise."""
    out = []
    for h in range(7):
        for tx in TXS:
            for itx, rc in FRAGS:
                for i in range(4):
                    out.append(G.BlockBody(INTS[i], INTS[(i + 1) % 4], INTS[(i + 2) % 4], HASHES[h],
                                           HASHES[(h + 2) % 7], HASHES[(h + 4) % 7], tx, itx, rc))
    return out


def hash_product_bodies() -> List[G.BlockBody]:
    """All 7^3 combinations of the three hashes (one setting of the rest)."""
    return [G.BlockBody(7, 8, 9, a, b, c, [b"tx"], None, None) for a in HASHES for b in HASHES for c in HASHES]


def random_bodies(n: int, seed: int) -> List[G.BlockBody]:
    rng = random.Random(seed)

    def rb(k):
        return bytes(rng.getrandbits(8) for _ in range(k))

    def rint():
        c = rng.random()
        if c < 0.3:
            return rng.choice(INTS + [1, 9, 10, 99, 100, 1_600_000_000])
        return rng.getrandbits(64) - 2**63

    def rhash():
        c = rng.random()
        return None if c < 0.15 else rb(rng.choice([0, 1, 2, 3, 31, 32, 33, 64]))

    def rtxs():
        c = rng.random()
        if c < 0.1:
            return None
        return [None if rng.random() < 0.1 else rb(rng.choice([0, 1, 2, 3, 4, 5, 63, 64, 65, 200]))
                for _ in range(rng.choice([0, 1, 2, 3, 16]))]

    def ritx():
        c = rng.random()
        if c < 0.5:
            return None
        return [G.InternalTransaction(G.InternalTransactionBody(rng.randrange(3), G.Peer("a:%d" % rng.randrange(99),
                                                                                          "0X" + rb(4).hex().upper(),
                                                                                          "mé\"<" + str(i))),
                                      "%x|%x" % (rng.getrandbits(64), rng.getrandbits(64)))
                for i in range(rng.randrange(3))]

    out = []
    for _ in range(n):
        itx = ritx()
        rc = None if rng.random() < 0.5 else [G.InternalTransactionReceipt(t, rng.random() < 0.5) for t in (ritx() or [])]
        out.append(G.BlockBody(rint(), rint(), rint(), rhash(), rhash(), rhash(), rtxs(), itx, rc))
    return out


def padded_body(target_len: int, mod: int = 64) -> G.BlockBody:
    """A body with ONE transaction sized so that len(Marshal()) % mod ==
    target_len % mod (base64 moves the length in steps of 4, the Timestamp's
    digits fill the rest)."""
    for ts_digits in range(1, 5):
        for tx_len in range(0, 3 * mod, 3):
            b = G.BlockBody(1, 2, 10 ** (ts_digits - 1), b"s", b"f", b"p", [bytes(tx_len)], None, None)
            if len(b.Marshal()) % mod == target_len % mod:
                return b
    raise AssertionError(target_len)


def body_of_length(n: int) -> G.BlockBody:
    """A body of exactly n bytes: one transaction, the Timestamp's digits fill in."""
    for ts_digits in range(1, 5):
        base = len(G.BlockBody(1, 2, 10 ** (ts_digits - 1), b"s", b"f", b"p", [b""], None, None).Marshal())
        rest = n - base
        if rest >= 0 and rest % 4 == 0:
            b = G.BlockBody(1, 2, 10 ** (ts_digits - 1), b"s", b"f", b"p", [bytes(rest // 4 * 3)], None, None)
            assert len(b.Marshal()) == n
            return b
    raise AssertionError(n)


# ----------------------------------------------------------------------------
# validators and signatures
# ----------------------------------------------------------------------------
_keys = {}
_pool = None


def validators(n: int):
    """n (private scalar, 65-byte public key) pairs, the same for every caller."""
    for i in range(n):
        if i not in _keys:
            d = int.from_bytes(hashlib.sha256(b"validator %d" % i).digest(), "big") % (G.N - 1) + 1
            _keys[i] = (d, G.Marshal(G.scalar_mult(d, G.G)))
    return [_keys[i] for i in range(n)]


def _nonce_pool():
    global _pool
    if _pool is None:
        _pool = []
        for j in range(4):
            k = int.from_bytes(hashlib.sha256(b"nonce %d" % j).digest(), "big") % (G.N - 1) + 1
            r = G.scalar_mult(k, G.G)[0] % G.N
            _pool.append((r, pow(k, -1, G.N)))
    return _pool


def sign(d: int, digest: bytes, j: int = 0) -> str:
    """The Signature text (keys.EncodeSignature) of a valid signature by d."""
    r, kinv = _nonce_pool()[j % 4]
    s = kinv * (int.from_bytes(digest, "big") + r * d) % G.N
    return G.EncodeSignature(r, s)


class BlockCase:
    """Bodies, their oracle bytes and digests, signatures as items, the packed
    field batch and the text batch over the ORACLE's serialised bodies."""

    def __init__(self, bodies: Sequence[G.BlockBody], items, n_validators: int, extra_keys: Sequence[bytes] = ()):
        """items: (block index, key index, signature text) in the caller's
        order; key indices past n_validators name extra_keys."""
        self.bodies = list(bodies)
        self.raw = [b.Marshal() for b in self.bodies]
        self.digests = np.frombuffer(b"".join(hashlib.sha256(r).digest() for r in self.raw), np.uint8).reshape(-1, 32)
        keys = [pub for _, pub in validators(n_validators)] + list(extra_keys)
        kb = BlockBatchBuilder()
        for b in self.bodies:
            kb.add_block(b)
        for k in keys:  # every key, in order (key index = position)
            kb.add_key(k)
        for blk, key, text in items:
            kb.add_signature(blk, keys[key], text)
        self.fields: PackedBlockBatch = kb.pack()
        off = np.zeros(len(self.raw) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in self.raw])
        self.oracle_bodies = (np.frombuffer(b"".join(self.raw), np.uint8).copy(), off)
        self.text = self.fields.text_batch(self.oracle_bodies)
        self._oracle = None

    @property
    def n_items(self) -> int:
        return self.fields.n_items

    def host(self) -> PackedBatch:
        return self.text.decoded()

    def oracle(self):
        """coracle.verify_batch over the oracle's bodies (computed once)."""
        if self._oracle is None:
            from oracle import coracle

            self._oracle = coracle.verify_batch(self.host().as_dict())
        return self._oracle

    def valid_count(self) -> np.ndarray:
        _, st, _ = self.oracle()
        return np.bincount(self.fields.item_block[st == 1], minlength=len(self.bodies)).astype(np.uint32)


def signed_case(bodies: Sequence[G.BlockBody], per_block, n_validators: int, seed: int = 1, shuffle: bool = False,
                corrupt: float = 0.0) -> BlockCase:
    """Every block b signed by per_block(b) validators (an int, or a callable
    of the block index); `corrupt`: that share of the signatures gets another
    s (REJECT)."""
    rng = random.Random(seed)
    vs = validators(n_validators)
    raw = [b.Marshal() for b in bodies]
    items = []
    for b, r in enumerate(raw):
        dig = hashlib.sha256(r).digest()
        n = per_block(b) if callable(per_block) else per_block
        for v in rng.sample(range(n_validators), n):
            text = sign(vs[v][0], dig, rng.randrange(4))
            if rng.random() < corrupt:
                text = text[:-1] + ("1" if text[-1] != "1" else "2")
            items.append((b, v, text))
    if shuffle:
        rng.shuffle(items)
    return BlockCase(bodies, items, n_validators)


def synth_like_bodies(n_blocks: int, n_tx: int = 16, tx_bytes: int = 64, seed: int = 9) -> List[G.BlockBody]:
    """Bodies of the C5 shape (16 x 64-B transactions, 32-byte hashes)."""
    rng = np.random.default_rng(seed)
    ph = hashlib.sha256(b"peers").digest()
    out = []
    for b in range(n_blocks):
        tx = rng.integers(0, 256, (n_tx, tx_bytes), dtype=np.uint8)
        out.append(G.BlockBody(b, b + 1, 1_600_000_000 + b, hashlib.sha256(b"s%d" % b).digest(),
                               hashlib.sha256(b"f%d" % b).digest(), ph, [tx[i].tobytes() for i in range(n_tx)], [], []))
    return out
