"""Chosen-scalar edge vectors for the compact key-cache geometry KC18 (18-bit
signed windows x 8 over each GLV half, 9-bit sub-tables; test infrastructure
only).  The machinery is tests/edge_vectors.py's, unchanged: Geometry, pack,
class_value, window_classes, _Builder.add_halves, craft, direct_status.

The set:
  b/KC18/  GLV-half patterns of u2 for the 18 x 8 windows, made here.
           edge_vectors.family_b cannot be asked for this geometry: its
           round-trip bound SAFE_HALF_BITS - W (NWIN - 1) is 126 - 126 = 0 bits
           of the top window, and it calls pack(.., safe - 2), a shift by a
           negative count.  The loop below is family_b's for one geometry with
           that bound clamped at 0.  Windows 0..6 take every class of
           _SIGNED_CYCLE; the top window holds 2 live bits (128 - 126), of
           which the split's halves (< 2^127) use digits 0..3: it reaches
           `zero` and `one`.  A 67 MB table per key allows all four sign pairs
           per rotation (the 805 MB KC tables allowed one).
  from edge_vectors.vectors(): families d and e (the final check and the
           exceptional totals) and b/max/* (halves up to 2^127: top-window
           digits 2 and 3).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import edge_vectors as ev
from tests.edge_vectors import (LAMBDA, N, SAFE_HALF_BITS, SIGNED_CLASSES, Geometry, Vector, _Builder, _SIGNED_CYCLE,
                                class_value, direct_status, glv_halves, pack, window_classes)

KC18 = Geometry("KC18", 18, 8, 9, True, 128)
SAFE_TOP = max(0, SAFE_HALF_BITS - KC18.W * (KC18.NWIN - 1))  # 0: the top window stays empty but for a carry


def family_b_kc18(b: _Builder) -> None:
    """edge_vectors._Builder.family_b for the one geometry KC18."""
    g, rng, safe = KC18, b.rng, SAFE_TOP
    for v in range(len(_SIGNED_CYCLE)):
        for sp in range(4):
            k1, k2 = pack(g, v, rng, safe), pack(g, v + 5, rng, safe)
            s1, s2 = (-1 if sp & 1 else 1), (-1 if sp & 2 else 1)
            b.add_halves(f"b/{g.name}/rot{v}/{'+-'[sp & 1]}{'+-'[sp >> 1]}", s1 * k1, s2 * k2, geom=g.name)
    # top-window classes above the round-trip bound: kept when the split returns them
    for cls in SIGNED_CLASSES:
        if (1 << safe) <= class_value(g, cls) < (1 << g.top_live):
            for h in (0, 1):
                others = [pack(g, 3 + 5 * h, rng, max(0, safe - 2)), rng.getrandbits(64),
                          (0x3760 << 112) | rng.getrandbits(100)]
                k = pack(g, 1, rng, g.top_live, force={g.NWIN - 1: cls})
                tag = f"b/{g.name}/top-{cls}/k{h + 1}"
                for o in others:
                    pair = (o, k) if h else (k, o)
                    if glv_halves((pair[0] + pair[1] * LAMBDA) % N) == pair:
                        b.add_halves(tag, pair[0], pair[1], geom=g.name)
                        break
                else:
                    b.dropped.append((tag, 0 if h else k, k if h else 0))
    a, c = pack(g, 2, rng, safe), pack(g, 9, rng, safe)
    b.add_halves(f"b/{g.name}/k1=0", 0, c, geom=g.name)
    b.add_halves(f"b/{g.name}/k2=0", -a, 0, geom=g.name)
    b.add_halves(f"b/{g.name}/k1=k2", a, a, geom=g.name)
    b.add_halves(f"b/{g.name}/k1=-k2", c, -c, geom=g.name)
    for h in (0, 1):  # from-identity shapes of window 0 / window 1 of each half
        hi = rng.getrandbits(120 - 2 * g.W) << (2 * g.W)
        w0, w1 = rng.randrange(2, 1 << (g.W - 1)), rng.randrange(2, 1 << (g.W - 1))
        for name, k in (("w0=0,w1!=0", hi | w1 << g.W), ("w0!=0,w1=0", hi | w0), ("w0=0,w1=0", hi)):
            ks = [pack(g, 4 + h, rng, safe), pack(g, 6 + h, rng, safe)]
            ks[h] = k
            b.add_halves(f"b/{g.name}/k{h + 1}:{name}", ks[0], ks[1] if h else -ks[1], geom=g.name)


_OWN: Optional[_Builder] = None
_ALL: Optional[List[Vector]] = None
_STATUS: Optional[np.ndarray] = None


def own() -> _Builder:
    """The builder holding the b/KC18/ vectors (seeded: the same every time)."""
    global _OWN
    if _OWN is None:
        _OWN = _Builder()
        family_b_kc18(_OWN)
        assert len({v.tag for v in _OWN.out}) == len(_OWN.out)
    return _OWN


def vectors() -> List[Vector]:
    """b/KC18/*, then families d and e and b/max/* of edge_vectors.vectors()."""
    global _ALL
    if _ALL is None:
        taken = [v for v in ev.vectors() if v.family in "de" or v.tag.startswith("b/max/")]
        _ALL = list(own().out) + taken
        assert len({v.tag for v in _ALL}) == len(_ALL)
    return _ALL


def dropped() -> List[Tuple[str, int, int]]:
    return own().dropped


def direct_statuses() -> np.ndarray:
    """direct_status of every vector (computed once)."""
    global _STATUS
    if _STATUS is None:
        _STATUS = np.array([direct_status(v) for v in vectors()], np.uint8)
    return _STATUS


def batch(idx: Optional[Sequence[int]] = None, repeat: int = 1):
    """PackedBatch of the vectors (all, or those at `idx`), as
    edge_vectors.batch: one message per vector, keys de-duplicated by bytes."""
    from babble_amd.batch import BatchBuilder

    vs = vectors()
    bb = BatchBuilder()
    for i in (range(len(vs)) if idx is None else idx):
        v = vs[i]
        bb.add_item_raw(bb.add_msg(v.body), bb.add_key(v.pub), 0, v.r.to_bytes(32, "big"), v.s.to_bytes(32, "big"))
    b = bb.pack()
    if repeat > 1:
        b.item_msg, b.item_key = np.tile(b.item_msg, repeat), np.tile(b.item_key, repeat)
        b.r_be, b.s_be, b.pre = np.tile(b.r_be, (repeat, 1)), np.tile(b.s_be, (repeat, 1)), np.tile(b.pre, repeat)
    return b


def halves_classes():
    """Per window of KC18: the classes the magnitudes of the halves of all
    vectors() reach (the split's own halves, glv_halves)."""
    seen = [set() for _ in range(KC18.NWIN)]
    for v in vectors():
        for k in glv_halves(v.u2):
            for j, c in enumerate(window_classes(KC18, abs(k))):
                seen[j] |= c
    return seen
