"""Packed struct-of-arrays batches for the C ABI (bv_batch).

A batch holds N messages (canonical JSON bodies, hashed once each), K public
keys (raw bytes, validated on the device) and M signature items, each naming
a message and a key and carrying r, s (32-byte big-endian) plus the host
pre-class byte (keys.DecodeSignature result, see include/babbleverify.h).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from . import native


@dataclass
class PackedBatch:
    msg_bytes: np.ndarray          # u8
    msg_off: np.ndarray            # u64, n_msgs + 1
    key_bytes: np.ndarray          # u8
    key_off: np.ndarray            # u64, n_keys + 1
    item_msg: np.ndarray           # u32
    item_key: np.ndarray           # u32
    r_be: np.ndarray               # u8 [n, 32]
    s_be: np.ndarray               # u8 [n, 32]
    pre: Optional[np.ndarray]      # u8 [n] or None (all zero)

    @property
    def n_msgs(self) -> int:
        return len(self.msg_off) - 1

    @property
    def n_keys(self) -> int:
        return len(self.key_off) - 1

    @property
    def n_items(self) -> int:
        return len(self.item_msg)

    def as_dict(self) -> Dict[str, np.ndarray]:
        return dict(msg_bytes=self.msg_bytes, msg_off=self.msg_off, key_bytes=self.key_bytes,
                    key_off=self.key_off, item_msg=self.item_msg, item_key=self.item_key,
                    r_be=self.r_be, s_be=self.s_be, pre=self.pre)

    def message(self, m: int) -> bytes:
        return self.msg_bytes[self.msg_off[m]:self.msg_off[m + 1]].tobytes()

    def key(self, k: int) -> bytes:
        return self.key_bytes[self.key_off[k]:self.key_off[k + 1]].tobytes()


@dataclass
class PackedTextBatch:
    """A PackedBatch without r / s / pre: every item's Signature text instead
    (bv_text_batch; the library decodes it, on the device for bulk batches)."""
    msg_bytes: np.ndarray          # u8
    msg_off: np.ndarray            # u64, n_msgs + 1
    key_bytes: np.ndarray          # u8
    key_off: np.ndarray            # u64, n_keys + 1
    item_msg: np.ndarray           # u32
    item_key: np.ndarray           # u32
    sig_off: np.ndarray            # u64, n_items + 1 byte offsets into sig_text
    sig_text: np.ndarray           # u8: the items' "r|s" texts, concatenated

    @property
    def n_msgs(self) -> int:
        return len(self.msg_off) - 1

    @property
    def n_keys(self) -> int:
        return len(self.key_off) - 1

    @property
    def n_items(self) -> int:
        return len(self.item_msg)

    def signature(self, i: int) -> bytes:
        return self.sig_text[int(self.sig_off[i]):int(self.sig_off[i + 1])].tobytes()

    def decoded(self) -> PackedBatch:
        """The PackedBatch of the same items, their texts decoded on the host
        (bv_decode_signatures)."""
        pre, r, s = native.decode_signatures(self.sig_off, self.sig_text)
        return PackedBatch(self.msg_bytes, self.msg_off, self.key_bytes, self.key_off, self.item_msg,
                           self.item_key, r, s, pre)


_ZERO32 = bytes(32)


def _cat(chunks):
    off = np.zeros(len(chunks) + 1, np.uint64)
    if chunks:
        off[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    buf = np.frombuffer(b"".join(chunks), np.uint8).copy() if chunks else np.zeros(0, np.uint8)
    return buf, off


class BatchBuilder:
    """Incrementally builds a PackedBatch (pack) or a PackedTextBatch
    (pack_text, when every item was added with its text); keys are
    de-duplicated by bytes."""

    def __init__(self):
        self._msgs: List[bytes] = []
        self._keys: List[bytes] = []
        self._key_idx: Dict[bytes, int] = {}
        self._item_msg: List[int] = []
        self._item_key: List[int] = []
        self._r: List[bytes] = []
        self._s: List[bytes] = []
        self._pre: List[int] = []
        self._text: List[Optional[bytes]] = []  # add_item's signature text (None: add_item_raw)

    def add_msg(self, body: bytes) -> int:
        self._msgs.append(bytes(body))
        return len(self._msgs) - 1

    def add_key(self, pub: bytes) -> int:
        pub = bytes(pub)
        k = self._key_idx.get(pub)
        if k is None:
            k = len(self._keys)
            self._keys.append(pub)
            self._key_idx[pub] = k
        return k

    def add_item(self, msg: int, key: int, signature) -> int:
        """signature: the r|s text of EncodeSignature (DecodeSignature
        semantics).  The text is kept as it is: pack() decodes every kept
        text in ONE bv_decode_signatures call, pack_text() ships them."""
        if isinstance(signature, str):
            signature = signature.encode("utf-8")
        i = self.add_item_raw(msg, key, 0, _ZERO32, _ZERO32)  # (placeholders: pack() decodes the text)
        self._text[i] = bytes(signature)
        return i

    def add_item_raw(self, msg: int, key: int, pre: int, r_be: bytes, s_be: bytes) -> int:
        self._item_msg.append(msg)
        self._item_key.append(key)
        self._pre.append(pre)
        self._r.append(bytes(r_be))
        self._s.append(bytes(s_be))
        self._text.append(None)
        return len(self._item_msg) - 1

    def pack(self) -> PackedBatch:
        mb, mo = _cat(self._msgs)
        kb, ko = _cat(self._keys)
        n = len(self._item_msg)
        r = np.frombuffer(b"".join(self._r), np.uint8).reshape(n, 32).copy() if n else np.zeros((0, 32), np.uint8)
        s = np.frombuffer(b"".join(self._s), np.uint8).reshape(n, 32).copy() if n else np.zeros((0, 32), np.uint8)
        pre = np.array(self._pre, np.uint8)
        idx = [i for i, t in enumerate(self._text) if t is not None]
        if idx:  # add_item's texts, decoded together
            tb, to = _cat([self._text[i] for i in idx])
            pre[idx], r[idx], s[idx] = native.decode_signatures(to, tb)
        return PackedBatch(mb, mo, kb, ko, np.array(self._item_msg, np.uint32), np.array(self._item_key, np.uint32),
                           r, s, pre)

    def pack_text(self) -> PackedTextBatch:
        """The batch with the signature texts add_item was given instead of
        r / s / pre.  ValueError if an item came through add_item_raw."""
        if any(t is None for t in self._text):
            raise ValueError("pack_text: an item was added without its signature text (add_item_raw)")
        mb, mo = _cat(self._msgs)
        kb, ko = _cat(self._keys)
        tb, to = _cat(self._text)
        return PackedTextBatch(mb, mo, kb, ko, np.array(self._item_msg, np.uint32),
                               np.array(self._item_key, np.uint32), to, tb)


# ----------------------------------------------------------------------------
# blocks from their fields (bv_block_batch, bv_verify_blocks)
# ----------------------------------------------------------------------------
_BLOCK_DTYPES = (("index", np.int64), ("round_received", np.int64), ("timestamp", np.int64),
                 ("hash_off", np.uint64), ("hash_bytes", np.uint8), ("hash_nil", np.uint8),
                 ("tx_start", np.uint64), ("tx_off", np.uint64), ("tx_bytes", np.uint8),
                 ("tx_list_nil", np.uint8), ("tx_nil", np.uint8), ("itx_off", np.uint64), ("itx_json", np.uint8),
                 ("rcpt_off", np.uint64), ("rcpt_json", np.uint8), ("key_bytes", np.uint8), ("key_off", np.uint64),
                 ("item_block", np.uint32), ("item_key", np.uint32), ("sig_off", np.uint64), ("sig_text", np.uint8),
                 ("r_be", np.uint8), ("s_be", np.uint8), ("pre", np.uint8))


@dataclass
class PackedBlockBatch:
    """BlockBody fields of n blocks and their signatures as items over blocks
    and validator keys (bv_block_batch): the library builds and hashes every
    BlockBody.Marshal() itself.  The signatures are text (sig_off / sig_text)
    or, after decoded(), r_be / s_be / pre."""
    index: np.ndarray            # i64 [n]
    round_received: np.ndarray   # i64 [n]
    timestamp: np.ndarray        # i64 [n]
    hash_off: np.ndarray         # u64 [3 n + 1]: StateHash, FrameHash, PeersHash of each block
    hash_bytes: np.ndarray       # u8
    hash_nil: Optional[np.ndarray]      # u8 [3 n] or None (no nil hash)
    tx_start: np.ndarray         # u64 [n + 1]
    tx_off: np.ndarray           # u64 [n_tx + 1]
    tx_bytes: np.ndarray         # u8
    tx_list_nil: Optional[np.ndarray]   # u8 [n] or None
    tx_nil: Optional[np.ndarray]        # u8 [n_tx] or None
    itx_off: Optional[np.ndarray]       # u64 [n + 1] or None (all nil)
    itx_json: np.ndarray
    rcpt_off: Optional[np.ndarray]
    rcpt_json: np.ndarray
    key_bytes: np.ndarray        # u8
    key_off: np.ndarray          # u64 [n_keys + 1]
    item_block: np.ndarray       # u32 [n_items]
    item_key: np.ndarray         # u32 [n_items]
    sig_off: Optional[np.ndarray] = None   # u64 [n_items + 1]
    sig_text: Optional[np.ndarray] = None  # u8
    r_be: Optional[np.ndarray] = None      # u8 [n_items, 32]
    s_be: Optional[np.ndarray] = None
    pre: Optional[np.ndarray] = None

    @property
    def n_blocks(self) -> int:
        return len(self.index)

    @property
    def n_keys(self) -> int:
        return len(self.key_off) - 1

    @property
    def n_items(self) -> int:
        return len(self.item_block)

    def c_struct(self, keep: list) -> "native.BvBlockBatch":
        """The bv_block_batch of this batch; the arrays it points at (converted
        to the C dtypes where needed) are appended to `keep`."""
        def p(name, dt):
            a = getattr(self, name)
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a.ctypes.data if a.size else None

        b = native.BvBlockBatch()
        b.n_blocks, b.n_keys, b.n_items = self.n_blocks, self.n_keys, self.n_items
        text = self.sig_off is not None
        for name, dt in _BLOCK_DTYPES:
            if name in ("r_be", "s_be", "pre") and text:
                continue
            setattr(b, name, p(name, dt))
        if text and not b.sig_text:  # every signature empty: a valid pointer to zero bytes
            keep.append(np.zeros(1, np.uint8))
            b.sig_text = keep[-1].ctypes.data
        return b

    def body_lens(self) -> np.ndarray:
        """bv_block_body_lens: n + 1 offsets of the serialised bodies."""
        keep: list = []
        cb = self.c_struct(keep)
        off = np.zeros(self.n_blocks + 1, np.uint64)
        rc = native.lib().bv_block_body_lens(cb, off.ctypes.data)
        if rc != native.BV_OK:
            raise native.BvError(rc, "bv_block_body_lens")
        return off

    def bodies(self):
        """bv_block_bodies: (msg_bytes u8, msg_off u64 [n + 1]) — every
        BlockBody.Marshal(), built by the library's host serialiser."""
        off = self.body_lens()
        keep: list = []
        cb = self.c_struct(keep)
        out = np.zeros(int(off[-1]), np.uint8)
        rc = native.lib().bv_block_bodies(cb, off.ctypes.data, out.ctypes.data if out.size else None)
        if rc != native.BV_OK:
            raise native.BvError(rc, "bv_block_bodies")
        return out, off

    def decoded(self) -> "PackedBlockBatch":
        """The same batch with r_be / s_be / pre decoded on the host
        (bv_decode_signatures) instead of the signature text."""
        import dataclasses

        if self.sig_off is None:
            return self
        pre, r, s = native.decode_signatures(self.sig_off, self.sig_text)
        return dataclasses.replace(self, sig_off=None, sig_text=None, r_be=r, s_be=s, pre=pre)

    def text_batch(self, bodies=None) -> PackedTextBatch:
        """The bv_text_batch of the same items over serialised bodies
        (`bodies` = (msg_bytes, msg_off); default: bodies())."""
        mb, mo = self.bodies() if bodies is None else bodies
        return PackedTextBatch(mb, mo, self.key_bytes, self.key_off, self.item_block, self.item_key, self.sig_off,
                               self.sig_text)

    def staged_bytes(self) -> int:
        """Bytes bv_verify_blocks stages over PCIe for this batch."""
        return int(sum(np.asarray(getattr(self, name)).nbytes for name, _ in _BLOCK_DTYPES
                       if getattr(self, name) is not None))


def _fragment(items) -> bytes:
    """encoding/json of a slice of objects with .json() (or the fragment's
    bytes as they are); None (nil) -> b"", which the library writes as null."""
    if items is None:
        return b""
    if isinstance(items, (bytes, bytearray)):
        return bytes(items)
    return b"[" + b",".join(t.json() for t in items) + b"]"


class BlockBatchBuilder:
    """Incrementally builds a PackedBlockBatch: add_block(body) takes a
    BlockBody (hashgraph.BlockBody; any object with its fields), add_signature
    a BlockSignature's block, validator key bytes and Signature text.  Keys
    are de-duplicated by bytes."""

    def __init__(self):
        self._blocks = []
        self._keys: List[bytes] = []
        self._key_idx: Dict[bytes, int] = {}
        self._item_block: List[int] = []
        self._item_key: List[int] = []
        self._text: List[bytes] = []

    def add_block(self, body) -> int:
        txs = body.Transactions
        self._blocks.append((int(body.Index), int(body.RoundReceived), int(body.Timestamp),
                             [None if h is None else bytes(h) for h in (body.StateHash, body.FrameHash,
                                                                        body.PeersHash)],
                             None if txs is None else [None if t is None else bytes(t) for t in txs],
                             _fragment(body.InternalTransactions), _fragment(body.InternalTransactionReceipts)))
        return len(self._blocks) - 1

    def add_key(self, pub: bytes) -> int:
        pub = bytes(pub)
        k = self._key_idx.get(pub)
        if k is None:
            k = self._key_idx[pub] = len(self._keys)
            self._keys.append(pub)
        return k

    def add_signature(self, block_index: int, validator_bytes: bytes, signature_text) -> int:
        if isinstance(signature_text, str):
            signature_text = signature_text.encode("utf-8")
        self._item_block.append(int(block_index))
        self._item_key.append(self.add_key(validator_bytes or b""))
        self._text.append(bytes(signature_text))
        return len(self._item_block) - 1

    def pack(self) -> PackedBlockBatch:
        bl = self._blocks
        n = len(bl)
        hashes = [h for b in bl for h in b[3]]
        hb, ho = _cat([h or b"" for h in hashes])
        txs = [t for b in bl for t in (b[4] or [])]
        tx_start = np.zeros(n + 1, np.uint64)
        if n:
            tx_start[1:] = np.cumsum([len(b[4] or []) for b in bl], dtype=np.uint64)
        tb, to = _cat([t or b"" for t in txs])

        def frag(xs):
            if not any(xs):
                return None, np.zeros(0, np.uint8)
            buf, off = _cat(xs)
            return off, buf

        itx_off, itx_json = frag([b[5] for b in bl])
        rcpt_off, rcpt_json = frag([b[6] for b in bl])
        kb, ko = _cat(self._keys)
        st, so = _cat(self._text)
        return PackedBlockBatch(
            index=np.array([b[0] for b in bl], np.int64), round_received=np.array([b[1] for b in bl], np.int64),
            timestamp=np.array([b[2] for b in bl], np.int64), hash_off=ho, hash_bytes=hb,
            hash_nil=np.array([h is None for h in hashes], np.uint8) if any(h is None for h in hashes) else None,
            tx_start=tx_start, tx_off=to, tx_bytes=tb,
            tx_list_nil=np.array([b[4] is None for b in bl], np.uint8) if any(b[4] is None for b in bl) else None,
            tx_nil=np.array([t is None for t in txs], np.uint8) if any(t is None for t in txs) else None,
            itx_off=itx_off, itx_json=itx_json, rcpt_off=rcpt_off, rcpt_json=rcpt_json, key_bytes=kb, key_off=ko,
            item_block=np.array(self._item_block, np.uint32), item_key=np.array(self._item_key, np.uint32),
            sig_off=so, sig_text=st)
