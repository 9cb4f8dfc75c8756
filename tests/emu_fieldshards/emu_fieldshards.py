"""ctypes wrapper of tests/emu_fieldshards/_build/libbvemufieldshards.so: the
rebased ITX / fields serialisers (itxjson.h, bsigjson.h with EvjBases, ItxBases
and BsigBases: what k_itx_body_hash_rb, k_ev_body_hash_itx_rb and
k_ev_body_hash_fields_rb run per lane) and the rebased fold (ev_fold with an
ITX base: k_ev_compose_rb) on the host.  Test infrastructure only."""
from __future__ import annotations

import ctypes
import dataclasses
import os
import subprocess

import numpy as np

from tests.emu_shards import emu_shards

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_build", "libbvemufieldshards.so")
PLAN_EXE = os.path.join(_HERE, "_build", "planfuzz")
_lib = None

# the order of the bases array (emu_fieldshards.cpp)
BASES = ("ev", "tx", "txb", "ph", "itx", "str", "bsig", "sig", "val", "frag_itx", "frag_bsig")


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
        L = ctypes.CDLL(LIB)
        P, U = ctypes.c_void_p, ctypes.c_uint64
        L.emufs_itx_body_hash.argtypes = [P, U, P, P]
        L.emufs_ev_body_hash_itx.argtypes = [P, U, U, P, P]
        L.emufs_ev_body_hash_fields.argtypes = [P, U, U, P, P]
        L.emufs_compose.argtypes = [U, P, U, P, P, P, P, P, P]
        for f in (L.emufs_itx_body_hash, L.emufs_ev_body_hash_itx, L.emufs_ev_body_hash_fields, L.emufs_compose):
            f.restype = None
        _lib = L
    return _lib


def plan_exe() -> str:
    """The ASan + UBSan driver of bv_plan_event_fields_shards (its own main)."""
    subprocess.run(["make", "-s", "-C", _HERE, "plan"], check=True)
    return PLAN_EXE


def slice_itx(xb, a: int, z: int, hash_lo: int, hash_hi: int):
    """What shard [a, z) of an events.PackedEventItxBatch ships: COPIES of its
    slices, the values in them unchanged, and the bases as a dict (BASES).
    itx_start None (a fields batch without ITX fields) stays None."""
    ev, wb = emu_shards.slice_wire(xb.events, a, z, hash_lo, hash_hi)
    bases = dict.fromkeys(BASES, 0)
    bases.update(ev=int(wb[0]), tx=int(wb[1]), txb=int(wb[2]), frag_itx=int(wb[3]), frag_bsig=int(wb[4]), ph=int(wb[5]))
    nil = None if xb.itx_list_nil is None else xb.itx_list_nil[a:z].copy()
    if xb.itx_start is None:
        return dataclasses.replace(xb, events=ev, itx_list_nil=nil), bases
    i0, i1 = int(xb.itx_start[a]), int(xb.itx_start[z])
    s0, s1 = (int(xb.itx_str_off[4 * i0]), int(xb.itx_str_off[4 * i1])) if i1 > i0 else (0, 0)
    bases.update(itx=i0, str=s0)
    sl = dataclasses.replace(xb, events=ev, itx_start=xb.itx_start[a:z + 1].copy(), itx_list_nil=nil,
                             itx_type=xb.itx_type[i0:i1].copy(),
                             itx_str_off=xb.itx_str_off[4 * i0:4 * i1 + 1].copy() if i1 > i0
                             else np.zeros(1, np.uint64),
                             itx_str=xb.itx_str[s0:s1].copy())
    return sl, bases


def slice_fields(fb, a: int, z: int, hash_lo: int, hash_hi: int):
    """The same for an events.PackedEventFieldsBatch: its block-signature
    slices too.  bsig_val_off is shipped (and its base set) only when an entry
    of the shard is BSIG_VAL_BYTES."""
    ev, bases = slice_itx(fb.ev, a, z, hash_lo, hash_hi)
    j0, j1 = int(fb.bsig_start[a]), int(fb.bsig_start[z])
    g0, g1 = (int(fb.bsig_sig_off[j0]), int(fb.bsig_sig_off[j1])) if j1 > j0 else (0, 0)
    kind = None if fb.bsig_val_kind is None else fb.bsig_val_kind[j0:j1].copy()
    has_bytes = kind is not None and bool((kind == 1).any())
    v0, v1 = (int(fb.bsig_val_off[j0]), int(fb.bsig_val_off[j1])) if has_bytes else (0, 0)
    bases.update(bsig=j0, sig=g0, val=v0)
    sl = dataclasses.replace(
        fb, ev=ev, bsig_start=fb.bsig_start[a:z + 1].copy(),
        bsig_list_nil=None if fb.bsig_list_nil is None else fb.bsig_list_nil[a:z].copy(),
        bsig_index=fb.bsig_index[j0:j1].copy(),
        bsig_sig_off=fb.bsig_sig_off[j0:j1 + 1].copy() if j1 > j0 else np.zeros(1, np.uint64),
        bsig_sig=fb.bsig_sig[g0:g1].copy(), bsig_val_kind=kind,
        bsig_val_off=fb.bsig_val_off[j0:j1 + 1].copy() if has_bytes else None,
        bsig_val_bytes=fb.bsig_val_bytes[v0:v1].copy())
    return sl, bases


def _bases(bases: dict) -> np.ndarray:
    return np.array([bases[k] for k in BASES], np.uint64)


def ev_body_hash(sl, bases: dict, a: int, z: int) -> np.ndarray:
    """Digests [z - a, 32] of events [a, z) from the shard's slices alone
    (`sl`: a sliced PackedEventItxBatch or PackedEventFieldsBatch)."""
    keep: list = []
    cb = sl.c_struct(keep)
    dig = np.zeros((max(z - a, 1), 32), np.uint8)
    b = _bases(bases)
    fn = lib().emufs_ev_body_hash_fields if hasattr(sl, "bsig_start") else lib().emufs_ev_body_hash_itx
    fn(ctypes.addressof(cb), a, z, b.ctypes.data, dig.ctypes.data)
    return dig[: z - a]


def itx_body_hash(sl, bases: dict) -> np.ndarray:
    """Digests [n_itx, 32] of the shard's ITXs from its slices alone (`sl`: a
    sliced PackedEventItxBatch)."""
    keep: list = []
    cb = sl.c_struct(keep)
    m = sl.n_itx
    dig = np.zeros((max(m, 1), 32), np.uint8)
    b = _bases(bases)
    lib().emufs_itx_body_hash(ctypes.addressof(cb), m, b.ctypes.data, dig.ctypes.data)
    return dig[:m]


def compose(itx_start_slice, itx_base: int, item_status, force):
    """k_ev_compose_rb over one shard: (event status, decided_by, accept words,
    itx status) from the shard's slice of itx_start (the whole batch's values)
    and its own item statuses (its events', then its ITXs') and force flags."""
    s = np.ascontiguousarray(itx_start_slice, np.uint64)
    n = len(s) - 1
    m = int(s[n]) - int(s[0])
    ist = np.ascontiguousarray(item_status, np.uint8)
    fp = np.ascontiguousarray(np.concatenate([np.asarray(force, np.uint8), np.zeros(1, np.uint8)]))
    assert len(ist) == n + m and len(fp) == m + 1
    st, by = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32)
    bits, its = np.zeros(max((n + 63) // 64, 1), np.uint64), np.zeros(max(m, 1), np.uint8)
    lib().emufs_compose(n, s.ctypes.data, itx_base, ist.ctypes.data, fp.ctypes.data, st.ctypes.data, by.ctypes.data,
                        bits.ctypes.data, its.ctypes.data)
    return st[:n], by[:n], bits[: (n + 63) // 64], its[:m]
