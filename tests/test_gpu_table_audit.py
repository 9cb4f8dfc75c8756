"""Every required entry of every fixed-base table, audited on the device.

Window j of a table for the point Q holds T[j][d] = d 2^(W j) Q.  The audit
kernels of tests/tablecheck/libtablecheck.so check, for every entry a verify
kernel can read, the relations of tests/tablecheck/audit.h: the anchor
(T[0][1] is the key), the step (T[j][d] = T[j][d-1] + T[j][1]), the link
between windows, canonical form, and the phi half.  All of them holding means
every entry is the multiple it must be, by induction from the key.  The
tables are the ones the library's own builders write: bvk::build_tables for
every per-batch variant it can pick, bvk::build_kc, and through the product's
orchestration the generator table and the cached key tables of live contexts.

A spot check against Python integers (oracle.gosemantics.scalar_mult) guards
against a vacuous audit, the audited count is held to the required-digit
formula, and a negative control corrupts single entries.  The relations are
tested against themselves on the CPU by tests/test_table_audit.py.
Run on the GPU box:
    python -u -m pytest tests/test_gpu_table_audit.py -m gpu -x -v
"""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle import gosemantics as gs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "tablecheck", "libtablecheck.so")
P, N = gs.P, gs.N
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
R0, R1, R2, R3, R4 = range(5)
KS_OK, KS_BAD = 0, 2
# kw -> (window bits, windows, scalar bits, signed digits, stored phi half)
GEOM = {0: (26, 10, 256, True, False), 8: (8, 16, 128, False, True), 12: (12, 11, 128, True, True),
        22: (22, 6, 128, True, False), 18: (18, 8, 128, True, False)}
# required entries per half, as the issue states them
REQUIRED = {0: 9 * 2 ** 25 + 2 ** 22, 8: 16 * 255, 12: 10 * 2 ** 11 + 2 ** 8, 22: 5 * 2 ** 21 + 2 ** 18,
            18: 7 * 2 ** 17 + 2 ** 2}
KNOBS = ("BV_K12_LAT", "BV_K8_DIRECT_KEYS", "BV_COOP_BASES")  # read once at library load: they pick the variant


class Result(ctypes.Structure):
    _fields_ = [("failures", ctypes.c_uint64), ("audited", ctypes.c_uint64), ("changed", ctypes.c_uint64),
                ("n_rec", ctypes.c_uint32), ("audit_ms", ctypes.c_float), ("rec", ctypes.c_uint32 * 256),
                ("err", ctypes.c_char * 160)]

    def records(self):
        return [tuple(self.rec[4 * i:4 * i + 4]) for i in range(self.n_rec)]


_LIB = None


@pytest.fixture(autouse=True)
def no_variant_knobs():
    for k in KNOBS:
        assert k not in os.environ, f"{k} is set: it would change which build variant runs"


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB):
            pytest.fail("tests/tablecheck/libtablecheck.so missing: run __graft_entry__.build()")
        from babble_amd import native

        native.lib()  # the product library first: the harness links it
        L = ctypes.CDLL(LIB)
        V, U32, U64, RP = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(Result)
        L.tc_build_audit.argtypes = [ctypes.c_int, U32, V, V, U64, U32, V, V, V, RP]
        L.tc_corrupt_audit.argtypes = [ctypes.c_int, U32, V, V, U32, U32, U32, U64, RP]
        L.tc_audit_ctx_g.argtypes = [V, V, U32, V, V, RP]
        L.tc_audit_ctx_kc.argtypes = [V, U32, V, V, V, U32, V, V, V, RP]
        for f in (L.tc_build_audit, L.tc_corrupt_audit, L.tc_audit_ctx_g, L.tc_audit_ctx_kc):
            f.restype = ctypes.c_int
        _LIB = L
    return _LIB


# --------------------------------------------------------------------------- geometry, in Python integers
def required(kw, j):
    """The largest digit window j must hold (audit.h has the derivation)."""
    w, nwin, bits, signed, _ = GEOM[kw]
    if not signed:
        return 2 ** w - 1
    return min(2 ** (w - 1), 2 ** (bits - w * j))


def slot_of(kw, j, d):
    w, _, _, signed, _ = GEOM[kw]
    ent = 2 ** (w - 1) if signed else 2 ** w
    return (j + 1) * ent if signed and d == ent else j * ent + d


def slot_scalar(kw, slot):
    """The multiple of the key a slot holds."""
    w, _, _, signed, _ = GEOM[kw]
    if not signed:
        j, d = divmod(slot, 2 ** w)
        return d << (w * j)
    ent = 2 ** (w - 1)
    j, d = divmod(slot, ent)
    return d << (w * j) if d else ent << (w * (j - 1))


def test_required_counts_match_the_formula():
    for kw, (w, nwin, bits, signed, _) in GEOM.items():
        assert sum(required(kw, j) for j in range(nwin)) == REQUIRED[kw]
        assert all(required(kw, j) == 2 ** (w - 1) for j in range(nwin - 1)) or not signed


def spot_slots(kw, rng, n_random=4):
    """Digit 1 and the largest required digit of every window (the top
    window's is its last required digit; a signed inner window's lives in slot
    0 of the next window), and seeded random required slots."""
    nwin = GEOM[kw][1]
    s = []
    for j in range(nwin):
        s += [slot_of(kw, j, 1), slot_of(kw, j, required(kw, j))]
    for _ in range(n_random):
        j = rng.randrange(nwin)
        s.append(slot_of(kw, j, rng.randrange(1, required(kw, j) + 1)))
    return s


# --------------------------------------------------------------------------- keys
_NAMED, _MORE = {}, []


def named():
    """G, -G, a seeded random key (R), a seeded key whose x has a top limb of
    all ones (T), and the key the skipped slot gets (S)."""
    if not _NAMED:
        rng = random.Random(0xF111)
        r = gs.scalar_mult(rng.randrange(1, N), gs.G)
        while True:
            t = gs.scalar_mult(rng.randrange(1, N), gs.G)
            if t[0] >> 248 == 0xFF:
                break
        _NAMED.update({"G": gs.G, "-G": (gs.GX, P - gs.GY), "R": r, "T": t,
                       "S": gs.scalar_mult(rng.randrange(1, N), gs.G)})
    return _NAMED


def keys(n):
    """G, -G, R, T, then distinct seeded keys up to n (each the last plus a
    fixed point: one addition instead of a scalar multiplication)."""
    nm = named()
    if not _MORE:
        rng = random.Random(0x30BE)
        _MORE.append(gs.scalar_mult(rng.randrange(1, N), gs.G))  # the step
        _MORE.append(gs.scalar_mult(rng.randrange(1, N), gs.G))
    while len(_MORE) < n:
        _MORE.append(gs.point_add(_MORE[-1], _MORE[0]))
    return ([nm["G"], nm["-G"], nm["R"], nm["T"]] + _MORE[1:])[:n]


def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def pack_kxy(pts):
    return np.array([words(x) + words(y) for x, y in pts], dtype=np.uint32)


def value(w):
    return sum(int(w[i]) << (32 * i) for i in range(8))


def check_spots(kw, pts, gkey, gslot, gout):
    """The gathered entries against scalar_mult of each slot's scalar."""
    phi = GEOM[kw][4]
    memo = {}
    for i, (k, s) in enumerate(zip(gkey, gslot)):
        if (k, s) not in memo:
            memo[(k, s)] = gs.scalar_mult(slot_scalar(kw, s), pts[k])
        want = memo[(k, s)]
        e = gout[i]
        assert (value(e[0:8]), value(e[8:16])) == want, (kw, k, s)
        if phi:
            assert (value(e[16:24]), value(e[24:32])) == (BETA * want[0] % P, want[1]), (kw, k, s, "phi")
    return len(memo)


def run_build(kw, pts, status, n_items, spot_keys, seed):
    rng = random.Random(seed)
    gkey, gslot = [], []
    for k in spot_keys:
        assert status[k] == KS_OK
        for s in spot_slots(kw, rng):
            gkey.append(k)
            gslot.append(s)
    kxy = pack_kxy(pts)
    kst = np.array(status, dtype=np.uint8)
    gk, gsl = np.array(gkey, dtype=np.uint32), np.array(gslot, dtype=np.uint64)
    gout = np.zeros((len(gkey), 32), dtype=np.uint32)
    res = Result()
    rc = lib().tc_build_audit(kw, len(pts), kxy.ctypes.data, kst.ctypes.data, n_items, len(gkey), gk.ctypes.data,
                              gsl.ctypes.data, gout.ctypes.data, ctypes.byref(res))
    assert rc == 0, (rc, res.err)
    print(f"kw {kw} keys {len(pts)} items {n_items}: audited {res.audited} failures {res.failures} "
          f"changed {res.changed} audit {res.audit_ms:.3f} ms")
    assert res.failures == 0, res.records()
    assert res.changed == 0, "a guard region or a skipped key's table was written"
    n_ok = sum(1 for s in status if s == KS_OK)
    assert res.audited == n_ok * (2 if GEOM[kw][4] else 1) * REQUIRED[kw]
    n = check_spots(kw, pts, gkey, gslot, gout)
    assert n <= 400
    return res


# (kw, keys, n_items): the smallest shape that selects each variant of
# bvk::build_tables / bvk::build_kc.  keys: a count (G, -G, R, T, then seeded
# keys) or the named keys; "S" is a key with a non-OK status, which the builders
# skip (in the middle, where a case has room for it).
VARIANTS = {
    "k8_direct": (8, ["G", "-G", "S", "R", "T"], 1),        # k_table_fill<8, 16, true>
    "k8_chord_w1_zipped": (8, 25, 1),       # k_table_pair_u<.., 1>, zipped sub-table fill
    "k8_chord_w1_plain": (8, 25, 131073),   # the same, plain fill (past BV_LAT_MAX_ITEMS)
    "k8_chord_w4": (8, 65, 1),              # k_table_pair_u<.., 4>
    "k8_chord_w16": (8, (257, 128), 1),     # k_table_pair_u<.., 16>: one inversion per key; 128 MiB; key 128 skipped
    "k12_zipped": (12, ["G", "-G", "S", "T"], 1),           # k_table_fill<6, 22> per entry, k_table_pair
    "k12_shared": (12, ["G", "R", "S", "T"], 131073),       # k_fill_multiples + k_table_fill_shared, k_table_pair
    "kc18": (18, ["-G", "S", "T"], 0),                      # build_kc, k_table_pair_kc<18, 9, 8>
    "kc": (22, ["R", "T"], 0),                              # build_kc, k_table_pair_kc<22, 11, 6>
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_build_variant(name):
    kw, ks, n_items = VARIANTS[name]
    if isinstance(ks, list):
        pts = [named()[k] for k in ks]
        status = [KS_BAD if k == "S" else KS_OK for k in ks]
        spot = [i for i, k in enumerate(ks) if k != "S"]
    else:
        n_keys, skipped = ks if isinstance(ks, tuple) else (ks, None)
        pts = list(keys(n_keys))
        status = [KS_OK] * n_keys
        spot = [0, 1, 3, n_keys - 1]  # G, -G, T and the last key
        if skipped is not None:
            pts[skipped] = named()["S"]
            status[skipped] = KS_BAD
            spot = [0, 3, skipped + 1, n_keys - 1]  # and the key after the skipped one
    assert len(set(pts)) == len(pts)
    run_build(kw, pts, status, n_items, spot, seed=kw * 1000003 + len(pts) * 131 + n_items)


# --------------------------------------------------------------------------- through the product's orchestration
def ctx_result(rc, res, n_keys, kw):
    assert rc == 0, (rc, res.err)
    print(f"kw {kw} keys {n_keys}: audited {res.audited} failures {res.failures} audit {res.audit_ms:.3f} ms")
    assert res.failures == 0, res.records()
    assert res.audited == n_keys * REQUIRED[kw]


def test_generator_table_of_a_context():
    """All 10 windows of the 21.5 GB generator table; 4 spot checks per window,
    slot 1 and the last required slot among them, so windows 8 and 9 (word
    offsets past 2^32) are compared with Python integers too."""
    from babble_amd.verifier import Verifier

    L = lib()
    rng = random.Random(0x6AB1E)
    gslot = []
    for j in range(10):
        top = required(0, j)
        gslot += [slot_of(0, j, 1), slot_of(0, j, top), slot_of(0, j, rng.randrange(2, top)),
                  slot_of(0, j, rng.randrange(2, top))]
    assert min(s * 16 for s in gslot if s >= 8 * 2 ** 25) >= 2 ** 32
    gsl = np.array(gslot, dtype=np.uint64)
    gout = np.zeros((len(gslot), 32), dtype=np.uint32)
    kxy = pack_kxy([gs.G])
    v = Verifier(device=0)
    try:
        res = Result()
        rc = L.tc_audit_ctx_g(v._ctx, kxy.ctypes.data, len(gslot), gsl.ctypes.data, gout.ctypes.data, ctypes.byref(res))
        ctx_result(rc, res, 1, 0)
    finally:
        v.close()
    assert check_spots(0, [gs.G], [0] * len(gslot), gslot, gout) == len(set(gslot))


def cached_context(flags, kw, n_keys, spot_keys):
    from babble_amd.verifier import Verifier

    L = lib()
    pts = list(keys(n_keys))
    raw = [gs.Marshal(q) for q in pts]
    assert len(set(raw)) == n_keys
    rng = random.Random(0xCAC4E + kw)
    gkey, gslot = [], []
    for k in spot_keys:
        for s in spot_slots(kw, rng):
            gkey.append(k)
            gslot.append(s)
    kb = np.frombuffer(b"".join(raw), dtype=np.uint8)
    ko = np.cumsum([0] + [len(r) for r in raw]).astype(np.uint64)
    kxy = pack_kxy(pts)
    gk, gsl = np.array(gkey, dtype=np.uint32), np.array(gslot, dtype=np.uint64)
    gout = np.zeros((len(gkey), 32), dtype=np.uint32)
    v = Verifier(device=0, flags=flags)
    try:
        v.register_keys(raw)
        v.sync()
        t = v.timing()
        assert t["kc_builds"] == n_keys == t["kc_keys"], t
        res = Result()
        rc = L.tc_audit_ctx_kc(v._ctx, n_keys, kb.ctypes.data, ko.ctypes.data, kxy.ctypes.data, len(gkey),
                               gk.ctypes.data, gsl.ctypes.data, gout.ctypes.data, ctypes.byref(res))
        ctx_result(rc, res, n_keys, kw)
        # a key the context never saw is an error, not an empty audit
        other = gs.Marshal(gs.scalar_mult(0xABCDEF, gs.G))
        ob = np.frombuffer(other, dtype=np.uint8)
        oo = np.array([0, len(other)], dtype=np.uint64)
        assert L.tc_audit_ctx_kc(v._ctx, 1, ob.ctypes.data, oo.ctypes.data, kxy.ctypes.data, 0, None, None, None,
                                 ctypes.byref(Result())) != 0
    finally:
        v.close()
    assert check_spots(kw, pts, gkey, gslot, gout) <= 400


def test_compact_key_cache_tables_of_a_context():
    """70 registered keys: two build rounds of the 64-key group (4.7 GB);
    spot checks on both sides of the group boundary."""
    from babble_amd import native

    cached_context(native.F_KEY_CACHE | native.F_KC_COMPACT, 18, 70, [0, 63, 64, 69])


def test_key_cache_tables_of_a_context():
    """9 registered keys: two build rounds of the 8-key group (7.2 GB)."""
    from babble_amd import native

    cached_context(native.F_KEY_CACHE, 22, 9, [0, 7, 8, 3])


# --------------------------------------------------------------------------- negative control
C_FLIP_X, C_NEG_Y, C_SWAP_NEXT, C_NEXT_WINDOW, C_PHI_PLAIN_X = 1, 2, 3, 4, 5
MID = {8: (7, 100), 12: (5, 1000)}  # a middle window and a digit with 2 < d < dmax - 2


def expected(kind, key, j, d):
    """The relations that read the touched slots (tablecheck.hip: the plain
    half alone for the first two, both halves for the moves)."""
    return {
        C_FLIP_X: [(R1, key, j, d), (R1, key, j, d + 1), (R4, key, j, d)],
        C_NEG_Y: [(R1, key, j, d), (R1, key, j, d + 1), (R4, key, j, d)],
        C_SWAP_NEXT: [(R1, key, j, d), (R1, key, j, d + 1), (R1, key, j, d + 2)],
        C_NEXT_WINDOW: [(R1, key, j, d), (R1, key, j, d + 1)],
        C_PHI_PLAIN_X: [(R4, key, j, d)],
    }[kind]


def corrupt(kw, kind, j, d):
    pts = list(keys(3))[1:3]  # -G and the random key (K8: 2 keys take the direct path)
    kxy = pack_kxy(pts)
    kst = np.zeros(2, dtype=np.uint8)
    res = Result()
    rc = lib().tc_corrupt_audit(kw, 2, kxy.ctypes.data, kst.ctypes.data, kind, 1, j, d, ctypes.byref(res))
    assert rc == 0, (rc, res.err)
    assert res.changed == 0
    assert res.audited == 2 * 2 * REQUIRED[kw]
    return res


@pytest.mark.parametrize("kw", [8, 12])
@pytest.mark.parametrize("kind", [C_FLIP_X, C_NEG_Y, C_SWAP_NEXT, C_NEXT_WINDOW, C_PHI_PLAIN_X])
def test_corruption_is_reported(kw, kind):
    j, d = MID[kw]
    assert 2 < d < required(kw, j) - 2 and 0 < j < GEOM[kw][1] - 1
    res = corrupt(kw, kind, j, d)
    got = res.records()
    assert res.failures >= 1 and res.failures == len(got)
    allowed = {(R1, 1, j, d + i) for i in range(3)} | {(R4, 1, j, d), (R4, 1, j, d + 1)}
    assert set(got) <= allowed, got
    assert all(f[1] == 1 for f in got), "the untouched key reported a failure"
    assert got == sorted(expected(kind, 1, j, d)), got


def test_corrupt_top_digit_in_next_windows_slot_zero():
    j, top = 5, 2 ** 11
    res = corrupt(12, C_FLIP_X, j, top)
    assert res.records() == sorted([(R1, 1, j, top), (R2, 1, j + 1, 1), (R4, 1, j, top)]) and res.failures == 3
