"""Events from their wire fields (bv_verify_events, include/babbleverify.h):
the device builds each canonical EventBody (event.go:38-45), hashes it —
level by level when a parent is an earlier event of the same batch — and
verifies the creator's signature.  SURVEY §8f rows 1-2.

    b = EventBatchBuilder()
    k = b.add_key(creator_pubkey)
    e0 = b.add_event(k, index=0, timestamp=t, parents=[None, None], transactions=[tx], signature=sig)
    e1 = b.add_event(k, index=1, timestamp=t + 1, parents=[("event", e0), ("hash", h32)], ...)
    res = verifier.verify_events(b.pack())      # msg_hash = Event.Hash(), status per event

Parents follow Hashgraph.ReadWireInfo (hashgraph.go:1540-1595): None -> ""
(wire index < 0), ("hash", 32 bytes) -> "0X" + hex of a hash from the store,
("event", i) -> the hash of event i of this batch (i < the child's index).
InternalTransactions / BlockSignatures are given as their encoding/json
fragments (b"" = nil -> null); the ITX signatures themselves are verified
through bv_verify_batch items (Event.Verify's ITX loop), not here.

Or the InternalTransactions as objects (add_event(..., itxs=[...])) and
pack_itx(): a PackedEventItxBatch for Verifier.verify_events_itx
(bv_verify_events_itx), which builds and hashes the ITX JSON on the device,
verifies the ITX signatures too and folds them per event as Event.Verify does.
Or the BlockSignatures as objects too (add_event(..., bsigs=[...])) and
pack_fields(): a PackedEventFieldsBatch for Verifier.verify_events_fields
(bv_verify_events_fields), the whole Event from fields, no JSON at all.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import native

PARENT_NONE, PARENT_HASH, PARENT_EVENT = 0, 1, 2


class BvEventBatch(ctypes.Structure):
    P = ctypes.c_void_p
    _fields_ = [
        ("n_events", ctypes.c_uint64), ("n_keys", ctypes.c_uint32), ("key_bytes", P), ("key_off", P),
        ("creator", P), ("index", P), ("timestamp", P), ("parent_kind", P), ("parent_ref", P),
        ("n_parent_hashes", ctypes.c_uint64), ("parent_hashes", P), ("tx_start", P), ("tx_off", P),
        ("tx_bytes", P), ("tx_list_nil", P), ("tx_nil", P), ("itx_off", P), ("itx_json", P), ("bsig_off", P),
        ("bsig_json", P), ("r_be", P), ("s_be", P), ("pre", P), ("sig_off", P), ("sig_text", P),
    ]


@dataclass
class EventWireBatch:
    key_bytes: np.ndarray       # u8
    key_off: np.ndarray         # u64 [n_keys + 1]
    creator: np.ndarray         # u32 [n]
    index: np.ndarray           # i64 [n]
    timestamp: np.ndarray       # i64 [n]
    parent_kind: np.ndarray     # u8 [n, 2]
    parent_ref: np.ndarray      # u64 [n, 2]
    parent_hashes: np.ndarray   # u8 [m, 32]
    tx_start: np.ndarray        # u64 [n + 1]
    tx_off: np.ndarray          # u64 [n_tx + 1]
    tx_bytes: np.ndarray        # u8
    tx_list_nil: Optional[np.ndarray]  # u8 [n] or None
    tx_nil: Optional[np.ndarray]       # u8 [n_tx] or None
    itx_off: Optional[np.ndarray]      # u64 [n + 1] or None (all nil)
    itx_json: np.ndarray
    bsig_off: Optional[np.ndarray]
    bsig_json: np.ndarray
    r_be: np.ndarray            # u8 [n, 32]
    s_be: np.ndarray            # u8 [n, 32]
    pre: Optional[np.ndarray]   # u8 [n]
    # or the Event.Signature text (decoded on the device; r_be / s_be / pre
    # are then not sent): u64 [n + 1] offsets and the bytes
    sig_off: Optional[np.ndarray] = None
    sig_text: Optional[np.ndarray] = None

    @property
    def n_events(self) -> int:
        return len(self.creator)

    def c_struct(self, keep: list) -> BvEventBatch:
        def p(a, dt=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a if dt is None else a.astype(dt, copy=False))
            keep.append(a)
            return a.ctypes.data if a.size else None

        b = BvEventBatch()
        b.n_events = self.n_events
        b.n_keys = len(self.key_off) - 1
        b.key_bytes, b.key_off = p(self.key_bytes), p(self.key_off, np.uint64)
        b.creator, b.index, b.timestamp = p(self.creator, np.uint32), p(self.index, np.int64), p(self.timestamp,
                                                                                                 np.int64)
        b.parent_kind, b.parent_ref = p(self.parent_kind, np.uint8), p(self.parent_ref, np.uint64)
        b.n_parent_hashes = len(self.parent_hashes)
        b.parent_hashes = p(self.parent_hashes)
        b.tx_start, b.tx_off, b.tx_bytes = p(self.tx_start, np.uint64), p(self.tx_off, np.uint64), p(self.tx_bytes)
        b.tx_list_nil, b.tx_nil = p(self.tx_list_nil), p(self.tx_nil)
        b.itx_off, b.itx_json = p(self.itx_off, np.uint64), p(self.itx_json)
        b.bsig_off, b.bsig_json = p(self.bsig_off, np.uint64), p(self.bsig_json)
        if self.sig_text is not None:  # the text only (the library decodes it on the device)
            b.sig_off, b.sig_text = p(self.sig_off, np.uint64), p(self.sig_text)
            if not b.sig_text:  # all signatures empty: a valid non-null pointer to zero bytes
                keep.append(np.zeros(1, np.uint8))
                b.sig_text = keep[-1].ctypes.data
        else:
            b.r_be, b.s_be, b.pre = p(self.r_be), p(self.s_be), p(self.pre)
        return b

    def with_signature_text(self, text: np.ndarray, off: np.ndarray) -> "EventWireBatch":
        """The same events carrying their Signature text instead of r / s /
        pre (bv_event_batch sig_text)."""
        import dataclasses

        return dataclasses.replace(self, sig_off=np.asarray(off, np.uint64),
                                   sig_text=np.asarray(text, np.uint8))


Parent = Union[None, Tuple[str, Union[int, bytes]]]


class EventBatchBuilder:
    def __init__(self):
        self._keys: List[bytes] = []
        self._key_idx = {}
        self._ev = []
        self._hashes: List[bytes] = []
        self._itxs: List[Optional[list]] = []
        self._bsigs: List[Optional[list]] = []
        self._sig_text: List[Optional[bytes]] = []

    def add_key(self, pub: bytes) -> int:
        pub = bytes(pub)
        k = self._key_idx.get(pub)
        if k is None:
            k = self._key_idx[pub] = len(self._keys)
            self._keys.append(pub)
        return k

    def add_event(self, creator: int, index: int, timestamp: int, parents: Sequence[Parent],
                  transactions: Optional[Sequence[Optional[bytes]]], signature, itx_json: bytes = b"",
                  bsig_json: bytes = b"", itxs: Optional[Sequence] = None, bsigs: Optional[Sequence] = None) -> int:
        """`signature`: the Event.Signature text (decoded as
        keys.DecodeSignature) or a (pre, r_be, s_be) tuple.  `itxs`: the
        event's InternalTransactions as objects (Body.Type, Body.Peer.NetAddr
        / PubKeyHex / Moniker, Signature; None = a nil slice, [] = an empty
        one) for pack_itx(), which needs every signature as text and no
        itx_json.  `bsigs`: the event's BlockSignatures as objects (Validator
        bytes or None, Index, Signature; None = a nil slice) for
        pack_fields(), which takes no bsig_json either."""
        kinds, refs = [], []
        for p in parents:
            if p is None:
                kinds.append(PARENT_NONE)
                refs.append(0)
            elif p[0] == "hash":
                kinds.append(PARENT_HASH)
                refs.append(len(self._hashes))
                self._hashes.append(bytes(p[1]))
            else:
                kinds.append(PARENT_EVENT)
                refs.append(int(p[1]))
        if isinstance(signature, tuple):
            pre, r, s = signature
        else:
            pre, r, s = native.decode_signature(signature)
        self._itxs.append(None if itxs is None else list(itxs))
        self._bsigs.append(None if bsigs is None else list(bsigs))
        self._sig_text.append(None if isinstance(signature, tuple) else _go_bytes(signature))
        self._ev.append((creator, index, timestamp, kinds, refs,
                         None if transactions is None else [None if t is None else bytes(t) for t in transactions],
                         bytes(itx_json), bytes(bsig_json), pre, r, s))
        return len(self._ev) - 1

    def pack(self) -> EventWireBatch:
        n = len(self._ev)
        key_off = np.zeros(len(self._keys) + 1, np.uint64)
        key_off[1:] = np.cumsum([len(k) for k in self._keys], dtype=np.uint64)
        txs = [t for e in self._ev for t in (e[5] or [])]
        tx_start = np.zeros(n + 1, np.uint64)
        tx_start[1:] = np.cumsum([len(e[5] or []) for e in self._ev], dtype=np.uint64)
        tx_off = np.zeros(len(txs) + 1, np.uint64)
        tx_off[1:] = np.cumsum([len(t or b"") for t in txs], dtype=np.uint64)
        itx = [e[6] for e in self._ev]
        bsg = [e[7] for e in self._ev]

        def frag(xs):
            if not any(xs):
                return None, np.zeros(0, np.uint8)
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum([len(x) for x in xs], dtype=np.uint64)
            return off, np.frombuffer(b"".join(xs), np.uint8).copy()

        itx_off, itx_json = frag(itx)
        bsig_off, bsig_json = frag(bsg)
        return EventWireBatch(
            key_bytes=np.frombuffer(b"".join(self._keys), np.uint8).copy(), key_off=key_off,
            creator=np.array([e[0] for e in self._ev], np.uint32),
            index=np.array([e[1] for e in self._ev], np.int64),
            timestamp=np.array([e[2] for e in self._ev], np.int64),
            parent_kind=np.array([e[3] for e in self._ev], np.uint8).reshape(n, 2),
            parent_ref=np.array([e[4] for e in self._ev], np.uint64).reshape(n, 2),
            parent_hashes=np.frombuffer(b"".join(self._hashes), np.uint8).reshape(-1, 32).copy(),
            tx_start=tx_start, tx_off=tx_off, tx_bytes=np.frombuffer(b"".join(t or b"" for t in txs), np.uint8).copy(),
            tx_list_nil=np.array([e[5] is None for e in self._ev], np.uint8)
            if any(e[5] is None for e in self._ev) else None,
            tx_nil=np.array([t is None for t in txs], np.uint8) if any(t is None for t in txs) else None,
            itx_off=itx_off, itx_json=itx_json, bsig_off=bsig_off, bsig_json=bsig_json,
            r_be=np.frombuffer(b"".join(e[9] for e in self._ev), np.uint8).reshape(n, 32).copy(),
            s_be=np.frombuffer(b"".join(e[10] for e in self._ev), np.uint8).reshape(n, 32).copy(),
            pre=np.array([e[8] for e in self._ev], np.uint8))


    def pack_itx(self) -> "PackedEventItxBatch":
        """The events with their InternalTransactions as fields
        (bv_event_itx_batch): the event signatures as text, the ITXs' four
        strings as raw bytes."""
        if any(t is None for t in self._sig_text):
            raise ValueError("pack_itx needs every event signature as text")
        if any(e[6] for e in self._ev):
            raise ValueError("pack_itx takes the ITXs as objects (itxs=), not as itx_json")
        n = len(self._ev)
        sig_off = np.zeros(n + 1, np.uint64)
        sig_off[1:] = np.cumsum([len(t) for t in self._sig_text], dtype=np.uint64)
        ev = self.pack().with_signature_text(np.frombuffer(b"".join(self._sig_text), np.uint8).copy(), sig_off)
        flat = [t for l in self._itxs for t in (l or [])]
        itx_start = np.zeros(n + 1, np.uint64)
        itx_start[1:] = np.cumsum([len(l or []) for l in self._itxs], dtype=np.uint64)
        strs = [_go_bytes(x) for t in flat
                for x in (t.Body.Peer.NetAddr, t.Body.Peer.PubKeyHex, t.Body.Peer.Moniker, t.Signature)]
        str_off = np.zeros(len(strs) + 1, np.uint64)
        str_off[1:] = np.cumsum([len(x) for x in strs], dtype=np.uint64)
        return PackedEventItxBatch(
            events=ev, itx_start=itx_start,
            itx_list_nil=np.array([l is None for l in self._itxs], np.uint8)
            if any(l is None for l in self._itxs) else None,
            itx_type=np.array([int(t.Body.Type) & 0xFF for t in flat], np.uint8), itx_str_off=str_off,
            itx_str=np.frombuffer(b"".join(strs), np.uint8).copy())


    def pack_fields(self, itx_fields: Optional[bool] = None) -> "PackedEventFieldsBatch":
        """The events with every member as fields (bv_event_fields_batch):
        pack_itx()'s batch and the BlockSignatures given as objects.  A
        Validator equal to the creator's key bytes is BV_BSIG_VAL_CREATOR,
        other bytes BV_BSIG_VAL_BYTES, None BV_BSIG_VAL_NIL.  itx_fields:
        False leaves out the ITX arrays (itx_start NULL; the batch must carry
        no ITX), None does so when no event has one."""
        if any(e[7] for e in self._ev):
            raise ValueError("pack_fields takes the block signatures as objects (bsigs=), not as bsig_json")
        xb = self.pack_itx()
        n = len(self._ev)
        if itx_fields is None:
            itx_fields = xb.n_itx > 0
        if not itx_fields:
            if xb.n_itx:
                raise ValueError("itx_fields=False with InternalTransactions in the batch")
            nil = np.array([l is None for l in self._itxs], np.uint8)
            xb = PackedEventItxBatch(events=xb.events, itx_start=None, itx_list_nil=None if nil.all() else nil,
                                     itx_type=np.zeros(0, np.uint8), itx_str_off=None, itx_str=np.zeros(0, np.uint8))
        flat = [(t, self._keys[e[0]]) for e, l in zip(self._ev, self._bsigs) for t in (l or [])]
        start = np.zeros(n + 1, np.uint64)
        start[1:] = np.cumsum([len(l or []) for l in self._bsigs], dtype=np.uint64)
        sigs = [_go_bytes(t.Signature) for t, _ in flat]
        sig_off = np.zeros(len(flat) + 1, np.uint64)
        sig_off[1:] = np.cumsum([len(x) for x in sigs], dtype=np.uint64)
        kind = np.array([BSIG_VAL_NIL if t.Validator is None else BSIG_VAL_CREATOR if bytes(t.Validator) == ck
                         else BSIG_VAL_BYTES for t, ck in flat], np.uint8)
        vals = [bytes(t.Validator) if k == BSIG_VAL_BYTES else b"" for (t, _), k in zip(flat, kind)]
        val_off = np.zeros(len(flat) + 1, np.uint64)
        val_off[1:] = np.cumsum([len(x) for x in vals], dtype=np.uint64)
        has_bytes = bool((kind == BSIG_VAL_BYTES).any())
        return PackedEventFieldsBatch(
            ev=xb, bsig_start=start,
            bsig_list_nil=np.array([l is None for l in self._bsigs], np.uint8)
            if any(l is None for l in self._bsigs) else None,
            bsig_index=np.array([int(t.Index) for t, _ in flat], np.int64), bsig_sig_off=sig_off,
            bsig_sig=np.frombuffer(b"".join(sigs), np.uint8).copy(),
            bsig_val_kind=kind if kind.any() else None, bsig_val_off=val_off if has_bytes else None,
            bsig_val_bytes=np.frombuffer(b"".join(vals), np.uint8).copy())


def _go_bytes(s) -> bytes:
    """A Go string's bytes (a str is its UTF-8; lone surrogates escape raw bytes)."""
    return s.encode("utf-8", "surrogateescape") if isinstance(s, str) else bytes(s)


class BvEventItxBatch(ctypes.Structure):
    P = ctypes.c_void_p
    _fields_ = [("events", BvEventBatch), ("itx_start", P), ("itx_list_nil", P), ("itx_type", P),
                ("itx_str_off", P), ("itx_str", P)]


class BvEventItxOut(ctypes.Structure):
    _fields_ = [("itx_hash", ctypes.c_void_p), ("itx_status", ctypes.c_void_p), ("decided_by", ctypes.c_void_p)]


EV_ITX_INVALID = 4      # BV_EV_ITX_INVALID
EV_SELF = 0xFFFFFFFF    # BV_EV_SELF


@dataclass
class PackedEventItxBatch:
    """bv_event_itx_batch: an EventWireBatch (signature text, no itx_json) and
    the InternalTransactions of its events as fields."""
    events: EventWireBatch
    itx_start: np.ndarray                # u64 [n + 1]
    itx_list_nil: Optional[np.ndarray]   # u8 [n] or None (no nil list)
    itx_type: np.ndarray                 # u8 [n_itx]
    itx_str_off: np.ndarray              # u64 [4 * n_itx + 1]
    itx_str: np.ndarray                  # u8

    @property
    def n_events(self) -> int:
        return self.events.n_events

    @property
    def n_itx(self) -> int:
        return len(self.itx_type)

    def c_struct(self, keep: list) -> BvEventItxBatch:
        def p(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a).astype(dt, copy=False))
            keep.append(a)
            return a.ctypes.data if a.size else None

        b = BvEventItxBatch()
        b.events = self.events.c_struct(keep)
        b.itx_start, b.itx_list_nil = p(self.itx_start, np.uint64), p(self.itx_list_nil, np.uint8)
        b.itx_type, b.itx_str_off = p(self.itx_type, np.uint8), p(self.itx_str_off, np.uint64)
        b.itx_str = p(self.itx_str, np.uint8)
        return b

    def _bodies(self, lens_fn, bodies_fn, n) -> List[bytes]:
        keep: list = []
        cb = self.c_struct(keep)
        off = np.zeros(n + 1, np.uint64)
        rc = lens_fn(ctypes.byref(cb), off.ctypes.data)
        if rc != native.BV_OK:
            raise native.BvError(rc, "body lengths")
        out = np.zeros(max(int(off[n]), 1), np.uint8)
        rc = bodies_fn(ctypes.byref(cb), off.ctypes.data, out.ctypes.data)
        if rc != native.BV_OK:
            raise native.BvError(rc, "bodies")
        raw = out.tobytes()
        return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]

    def itx_bodies(self) -> List[bytes]:
        """bv_itx_bodies: InternalTransactionBody.Marshal() of every ITX (host only)."""
        L = native.lib()
        return self._bodies(L.bv_itx_body_lens, L.bv_itx_bodies, self.n_itx)

    def event_bodies(self) -> List[bytes]:
        """bv_event_itx_bodies: EventBody.Marshal() of every event, an
        in-batch parent's hash as 64 '0' (host only)."""
        L = native.lib()
        return self._bodies(L.bv_event_itx_body_lens, L.bv_event_itx_bodies, self.n_events)


BSIG_VAL_CREATOR, BSIG_VAL_BYTES, BSIG_VAL_NIL = 0, 1, 2   # BV_BSIG_VAL_*


class BvEventFieldsBatch(ctypes.Structure):
    P = ctypes.c_void_p
    _fields_ = [("ev", BvEventItxBatch), ("bsig_start", P), ("bsig_list_nil", P), ("bsig_index", P),
                ("bsig_sig_off", P), ("bsig_sig", P), ("bsig_val_kind", P), ("bsig_val_off", P), ("bsig_val_bytes", P)]


@dataclass
class PackedEventFieldsBatch:
    """bv_event_fields_batch: a PackedEventItxBatch (its itx_start None: no
    ITX fields) and the BlockSignatures of its events as fields."""
    ev: PackedEventItxBatch
    bsig_start: np.ndarray                # u64 [n + 1]
    bsig_list_nil: Optional[np.ndarray]   # u8 [n] or None (no nil list)
    bsig_index: np.ndarray                # i64 [n_bsig]
    bsig_sig_off: np.ndarray              # u64 [n_bsig + 1]
    bsig_sig: np.ndarray                  # u8
    bsig_val_kind: Optional[np.ndarray]   # u8 [n_bsig] or None (all the creator's key)
    bsig_val_off: Optional[np.ndarray]    # u64 [n_bsig + 1] or None (no BSIG_VAL_BYTES entry)
    bsig_val_bytes: np.ndarray            # u8

    @property
    def n_events(self) -> int:
        return self.ev.n_events

    @property
    def n_itx(self) -> int:
        return self.ev.n_itx

    @property
    def n_bsig(self) -> int:
        return len(self.bsig_index)

    def c_struct(self, keep: list) -> BvEventFieldsBatch:
        def p(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a).astype(dt, copy=False))
            keep.append(a)
            return a.ctypes.data if a.size else None

        b = BvEventFieldsBatch()
        b.ev = self.ev.c_struct(keep)
        b.bsig_start, b.bsig_list_nil = p(self.bsig_start, np.uint64), p(self.bsig_list_nil, np.uint8)
        b.bsig_index, b.bsig_sig_off = p(self.bsig_index, np.int64), p(self.bsig_sig_off, np.uint64)
        b.bsig_sig, b.bsig_val_kind = p(self.bsig_sig, np.uint8), p(self.bsig_val_kind, np.uint8)
        b.bsig_val_off, b.bsig_val_bytes = p(self.bsig_val_off, np.uint64), p(self.bsig_val_bytes, np.uint8)
        return b

    def event_bodies(self) -> List[bytes]:
        """bv_event_fields_bodies: EventBody.Marshal() of every event, an
        in-batch parent's hash as 64 '0' (host only)."""
        L = native.lib()
        return PackedEventItxBatch._bodies(self, L.bv_event_fields_body_lens, L.bv_event_fields_bodies, self.n_events)


def fields_bytes(fb: PackedEventFieldsBatch) -> int:
    """Bytes of the block-signature fields of this batch (what
    bv_verify_events_fields stages for them on its bulk path)."""
    arrs = [fb.bsig_start, fb.bsig_index, fb.bsig_sig_off, fb.bsig_sig, fb.bsig_val_bytes]
    arrs += [a for a in (fb.bsig_list_nil, fb.bsig_val_kind, fb.bsig_val_off) if a is not None]
    return int(sum(a.nbytes for a in arrs))


def wire_bytes(b: EventWireBatch) -> int:
    """Bytes bv_verify_events stages over PCIe for this batch."""
    arrs = [b.key_bytes, b.key_off, b.creator, b.index, b.timestamp, b.parent_kind, b.parent_ref, b.parent_hashes,
            b.tx_start, b.tx_off, b.tx_bytes, b.itx_json, b.bsig_json, b.r_be, b.s_be]
    arrs += [a for a in (b.tx_list_nil, b.tx_nil, b.itx_off, b.bsig_off, b.pre) if a is not None]
    return int(sum(a.nbytes for a in arrs))
