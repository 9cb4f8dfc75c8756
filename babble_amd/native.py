"""ctypes binding of libbabbleverify.so (include/babbleverify.h).

The product path: every verify goes through this library's gfx950 kernels.
If the library or a gfx950 device is missing the calls raise — there is no
CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbabbleverify.so")

BV_OK = 0
BV_E_ARGS = -1
BV_E_NODEVICE = -2
BV_E_OOM = -3
BV_E_LAUNCH = -4
BV_E_COMM = -5

REJECT, ACCEPT, REJECT_ERR, REF_PANIC = 0, 1, 2, 3
SC_OK, SC_NIL, SC_NONPOS, SC_GE_N = 0, 1, 2, 3
PRE_PARTS_BAD = 0x80
F_DEFAULT = 0
ABI_VERSION = 6
ARENA_SLOTS = 32
F_KEY_CACHE = 1
F_K8 = 2
F_KC_COMPACT = 4  # with F_KEY_CACHE: compact 18-bit cached tables (67.1 MB per key, 1430 in 96 GB)

# Every symbol include/babbleverify.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "bv_abi_version", "bv_create", "bv_destroy", "bv_last_error", "bv_verify_batch",
    "bv_verify_batch_device", "bv_sha256_batch", "bv_get_timing", "bv_decode_signature",
    "bv_hex_decode", "bv_group_create", "bv_group_destroy", "bv_group_last_error", "bv_group_verify_batch",
    "bv_group_get_timing", "bv_plan_shards", "bv_sync", "bv_peer_set_hash", "bv_verify_events",
    "bv_last_stream", "bv_host_alloc", "bv_host_free", "bv_merge_shard_bits", "bv_plan_group",
    "bv_kc_register", "bv_arena_create", "bv_arena_destroy", "bv_arena_reserve",
    "bv_group_verify_events", "bv_group_kc_register", "bv_plan_event_shards",
    "bv_kc_small_tables", "bv_verify_batch_text", "bv_decode_signatures",
    "bv_verify_blocks", "bv_block_body_lens", "bv_block_bodies",
    "bv_verify_events_itx", "bv_itx_body_lens", "bv_itx_bodies", "bv_event_itx_body_lens", "bv_event_itx_bodies",
    "bv_verify_events_fields", "bv_event_fields_body_lens", "bv_event_fields_bodies",
    "bv_group_verify_blocks", "bv_plan_block_shards",
    "bv_group_verify_events_itx", "bv_group_verify_events_fields", "bv_plan_event_fields_shards",
)


class BvBatch(ctypes.Structure):
    _fields_ = [
        ("n_msgs", ctypes.c_uint64),
        ("msg_bytes", ctypes.c_void_p),
        ("msg_off", ctypes.c_void_p),
        ("n_keys", ctypes.c_uint32),
        ("key_bytes", ctypes.c_void_p),
        ("key_off", ctypes.c_void_p),
        ("n_items", ctypes.c_uint64),
        ("item_msg", ctypes.c_void_p),
        ("item_key", ctypes.c_void_p),
        ("r_be", ctypes.c_void_p),
        ("s_be", ctypes.c_void_p),
        ("pre", ctypes.c_void_p),
    ]


class BvTextBatch(ctypes.Structure):
    _fields_ = [
        ("items", BvBatch),
        ("sig_off", ctypes.c_void_p),
        ("sig_text", ctypes.c_void_p),
    ]


class BvBlockBatch(ctypes.Structure):
    """bv_block_batch: BlockBody fields and the block signatures as items."""
    _P = ctypes.c_void_p
    _fields_ = [
        ("n_blocks", ctypes.c_uint64), ("index", _P), ("round_received", _P), ("timestamp", _P),
        ("hash_off", _P), ("hash_bytes", _P), ("hash_nil", _P),
        ("tx_start", _P), ("tx_off", _P), ("tx_bytes", _P), ("tx_list_nil", _P), ("tx_nil", _P),
        ("itx_off", _P), ("itx_json", _P), ("rcpt_off", _P), ("rcpt_json", _P),
        ("n_keys", ctypes.c_uint32), ("key_bytes", _P), ("key_off", _P),
        ("n_items", ctypes.c_uint64), ("item_block", _P), ("item_key", _P),
        ("sig_off", _P), ("sig_text", _P), ("r_be", _P), ("s_be", _P), ("pre", _P),
    ]


class BvResult(ctypes.Structure):
    _fields_ = [
        ("msg_hash", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("accept_bits", ctypes.c_void_p),
    ]


class BvTiming(ctypes.Structure):
    _fields_ = [
        ("ms_total", ctypes.c_float),
        ("ms_sha256", ctypes.c_float),
        ("ms_keyprep", ctypes.c_float),
        ("ms_scalar", ctypes.c_float),
        ("ms_verify_g", ctypes.c_float),
        ("ms_verify", ctypes.c_float),
        ("ms_h2d", ctypes.c_float),
        ("ms_d2h", ctypes.c_float),
        ("ms_host", ctypes.c_float),
        ("ms_host_prep", ctypes.c_float),
        ("ms_host_out", ctypes.c_float),
        ("key_path", ctypes.c_uint32),
        ("kc_hits", ctypes.c_uint32),
        ("kc_builds", ctypes.c_uint32),
        ("kc_keys", ctypes.c_uint32),
    ]


class BvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"babbleverify error {code}: {msg}")
        self.code = code


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BvError(BV_E_NODEVICE, f"{LIB_PATH} not built; run __graft_entry__.build()")
    # One HIP runtime per process: PyTorch-ROCm bundles its own
    # libamdhip64.so (soname libamdhip64.so.7).  Loading torch first makes
    # the dynamic loader resolve our NEEDED libamdhip64.so.7 to that same
    # runtime, so torch tensors (HBM plumbing, RCCL collectives) and our
    # kernels share one device context.  Without torch the library binds to
    # /opt/rocm's runtime (the cgo / plain C use).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    L.bv_abi_version.restype = ctypes.c_int
    L.bv_create.argtypes = [ctypes.POINTER(P), ctypes.c_int, ctypes.c_uint32]
    L.bv_create.restype = ctypes.c_int
    L.bv_destroy.argtypes = [P]
    L.bv_last_error.argtypes = [P]
    L.bv_last_error.restype = ctypes.c_char_p
    L.bv_verify_batch.argtypes = [P, ctypes.POINTER(BvBatch), ctypes.POINTER(BvResult)]
    L.bv_verify_batch.restype = ctypes.c_int
    L.bv_verify_batch_text.argtypes = [P, ctypes.POINTER(BvTextBatch), ctypes.POINTER(BvResult)]
    L.bv_verify_batch_text.restype = ctypes.c_int
    L.bv_decode_signatures.argtypes = [ctypes.c_uint64, P, P, P, P, P]
    L.bv_decode_signatures.restype = ctypes.c_int
    L.bv_verify_blocks.argtypes = [P, ctypes.POINTER(BvBlockBatch), ctypes.POINTER(BvResult), P]
    L.bv_verify_blocks.restype = ctypes.c_int
    L.bv_block_body_lens.argtypes = [ctypes.POINTER(BvBlockBatch), P]
    L.bv_block_body_lens.restype = ctypes.c_int
    L.bv_block_bodies.argtypes = [ctypes.POINTER(BvBlockBatch), P, P]
    L.bv_block_bodies.restype = ctypes.c_int
    L.bv_verify_batch_device.argtypes = [P, ctypes.POINTER(BvBatch), ctypes.POINTER(BvResult), P, ctypes.c_int]
    L.bv_verify_batch_device.restype = ctypes.c_int
    L.bv_sha256_batch.argtypes = [P, ctypes.c_uint64, P, P, P]
    L.bv_sha256_batch.restype = ctypes.c_int
    L.bv_get_timing.argtypes = [P, ctypes.POINTER(BvTiming)]
    L.bv_get_timing.restype = ctypes.c_int
    L.bv_decode_signature.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P, P]
    L.bv_decode_signature.restype = ctypes.c_uint8
    L.bv_hex_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P]
    L.bv_hex_decode.restype = ctypes.c_int64
    L.bv_group_create.argtypes = [ctypes.POINTER(P), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_uint32]
    L.bv_group_create.restype = ctypes.c_int
    L.bv_group_destroy.argtypes = [P]
    L.bv_group_last_error.argtypes = [P]
    L.bv_group_last_error.restype = ctypes.c_char_p
    L.bv_group_verify_batch.argtypes = [P, ctypes.POINTER(BvBatch), ctypes.POINTER(BvResult)]
    L.bv_group_verify_batch.restype = ctypes.c_int
    L.bv_group_get_timing.argtypes = [P, ctypes.c_int, ctypes.POINTER(BvTiming)]
    L.bv_group_get_timing.restype = ctypes.c_int
    L.bv_verify_events.argtypes = [P, P, ctypes.POINTER(BvResult)]
    L.bv_verify_events.restype = ctypes.c_int
    L.bv_verify_events_itx.argtypes = [P, P, ctypes.POINTER(BvResult), P]
    L.bv_verify_events_itx.restype = ctypes.c_int
    L.bv_verify_events_fields.argtypes = [P, P, ctypes.POINTER(BvResult), P]
    L.bv_verify_events_fields.restype = ctypes.c_int
    for f in (L.bv_itx_body_lens, L.bv_event_itx_body_lens, L.bv_event_fields_body_lens):
        f.argtypes = [P, P]
        f.restype = ctypes.c_int
    for f in (L.bv_itx_bodies, L.bv_event_itx_bodies, L.bv_event_fields_bodies):
        f.argtypes = [P, P, P]
        f.restype = ctypes.c_int
    L.bv_peer_set_hash.argtypes = [P, ctypes.c_uint32, P, P, P]
    L.bv_peer_set_hash.restype = ctypes.c_int
    L.bv_sync.argtypes = [P]
    L.bv_sync.restype = ctypes.c_int
    L.bv_plan_shards.argtypes = [ctypes.POINTER(BvBatch), ctypes.c_int, P]
    L.bv_plan_shards.restype = ctypes.c_int
    L.bv_last_stream.argtypes = [P]
    L.bv_last_stream.restype = P
    L.bv_host_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(P)]
    L.bv_host_alloc.restype = ctypes.c_int
    L.bv_host_free.argtypes = [P]
    L.bv_host_free.restype = None
    L.bv_merge_shard_bits.argtypes = [P, ctypes.c_uint64, ctypes.c_int, P, P]
    L.bv_merge_shard_bits.restype = ctypes.c_int
    L.bv_plan_group.argtypes = [ctypes.POINTER(BvBatch), ctypes.c_int, P, P, P]
    L.bv_plan_group.restype = ctypes.c_int
    L.bv_kc_register.argtypes = [P, ctypes.c_uint32, P, P]
    L.bv_kc_register.restype = ctypes.c_int
    L.bv_kc_small_tables.argtypes = [P, ctypes.c_int]
    L.bv_kc_small_tables.restype = ctypes.c_int
    L.bv_group_verify_events.argtypes = [P, P, ctypes.POINTER(BvResult)]
    L.bv_group_verify_events.restype = ctypes.c_int
    L.bv_group_kc_register.argtypes = [P, ctypes.c_uint32, P, P]
    L.bv_group_kc_register.restype = ctypes.c_int
    L.bv_plan_event_shards.argtypes = [P, ctypes.c_int, P, P, P]
    L.bv_plan_event_shards.restype = ctypes.c_int
    L.bv_group_verify_blocks.argtypes = [P, ctypes.POINTER(BvBlockBatch), ctypes.POINTER(BvResult), P]
    L.bv_group_verify_blocks.restype = ctypes.c_int
    L.bv_plan_block_shards.argtypes = [ctypes.POINTER(BvBlockBatch), ctypes.c_int, P, P]
    L.bv_plan_block_shards.restype = ctypes.c_int
    L.bv_group_verify_events_itx.argtypes = [P, P, ctypes.POINTER(BvResult), P]
    L.bv_group_verify_events_itx.restype = ctypes.c_int
    L.bv_group_verify_events_fields.argtypes = [P, P, ctypes.POINTER(BvResult), P]
    L.bv_group_verify_events_fields.restype = ctypes.c_int
    L.bv_plan_event_fields_shards.argtypes = [P, ctypes.c_int, P, P, P, P, P]
    L.bv_plan_event_fields_shards.restype = ctypes.c_int
    L.bv_arena_create.argtypes = [ctypes.POINTER(P)]
    L.bv_arena_create.restype = ctypes.c_int
    L.bv_arena_destroy.argtypes = [P]
    L.bv_arena_destroy.restype = None
    L.bv_arena_reserve.argtypes = [P, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(P),
                                   ctypes.POINTER(ctypes.c_size_t)]
    L.bv_arena_reserve.restype = ctypes.c_int
    if L.bv_abi_version() != ABI_VERSION:
        raise BvError(BV_E_ARGS, "ABI version mismatch")
    _lib = L
    return L


def decode_signature(sig: bytes):
    """bv_decode_signature: keys.DecodeSignature + pre-class -> (pre, r_be, s_be)."""
    if isinstance(sig, str):
        sig = sig.encode("utf-8")
    r = ctypes.create_string_buffer(32)
    s = ctypes.create_string_buffer(32)
    pre = lib().bv_decode_signature(sig, len(sig), r, s)
    return pre, r.raw, s.raw


def decode_signatures(sig_off, sig_text):
    """bv_decode_signatures: bv_decode_signature over len(sig_off) - 1 texts in
    one call -> (pre [n] u8, r_be [n, 32] u8, s_be [n, 32] u8)."""
    import numpy as np

    off = np.ascontiguousarray(sig_off, dtype=np.uint64)
    text = np.ascontiguousarray(sig_text, dtype=np.uint8)
    n = max(len(off) - 1, 0)
    if n and int(off[n]) > text.size:
        raise BvError(BV_E_ARGS, "sig_off runs past sig_text")
    r = np.zeros((n, 32), np.uint8)
    s = np.zeros((n, 32), np.uint8)
    pre = np.zeros(n, np.uint8)
    rc = lib().bv_decode_signatures(n, off.ctypes.data if n else None, text.ctypes.data if text.size else None,
                                    r.ctypes.data if n else None, s.ctypes.data if n else None,
                                    pre.ctypes.data if n else None)
    if rc != BV_OK:
        raise BvError(rc, "bv_decode_signatures")
    return pre, r, s


class ReferencePanic(Exception):
    """The Go reference would panic on this input (unrecovered in Babble)."""


def hex_decode(s) -> bytes:
    """bv_hex_decode: common.DecodeFromString semantics (partial prefix kept)."""
    if isinstance(s, str):
        s = s.encode("utf-8")
    out = ctypes.create_string_buffer(max(len(s) // 2, 1))
    n = lib().bv_hex_decode(s, len(s), out)
    if n < 0:
        raise ReferencePanic("slice bounds out of range in DecodeFromString")
    return out.raw[:n]
