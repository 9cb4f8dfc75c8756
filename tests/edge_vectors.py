"""Chosen-scalar ECDSA edge vectors (test infrastructure only).

Every end-to-end parity test feeds the verify paths signatures whose scalars
u1 = e / s and u2 = r / s are uniformly random, so the places where a
windowed, signed-digit, GLV-split verifier goes wrong (a zero digit, the digit
2^(W-1) kept in the next window's slot 0, a carry through every window, a
chord-sum entry with one identity operand, x(R) >= N, an empty GLV half, a
burst of NAF digits in k_small's first phase) are met with probability 2^-26
or less per item.  Any pair (u1, u2) can be forced exactly under a real
SHA-256 digest by public-key recovery:

    e = SHA-256(body),  s = e / u1,  r = u2 s  (mod N),
    R = a curve point with x(R) = r (or r + N),
    Q = u2^-1 (R - u1 G)

so u1 G + u2 Q = R and (r, s) verifies under Q.  Half of all r are the x of
a point; a counter in the body is stepped until r is.  Everything here is
Python integers over oracle.gosemantics' curve code, seeded, and cached in
the module: `vectors()` generates the set on first use (a few seconds).

Families (the tag of a vector starts with its family and names its pattern):
  a/  u1 patterns for the generator-table geometries 26x10 (product), 22x12
      (tests/emu) and 16x17 (the sanitized emulator)
  b/  GLV-half patterns of u2 for K12 (12x11), K8 (8x16) and KC (22x6)
  c/  NAF patterns of the halves for k_small's cold scheduler
  d/  the final check: x(R) = r + N (accepted only below p - N) and the
      vectors that only a missing or wrong `r < p - N` guard accepts
  e/  exceptional totals (u1 G = +-u2 Q) with recovered keys
"""
from __future__ import annotations

import hashlib
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import gosemantics as gs

P, N = gs.P, gs.N
ACCEPT, REJECT = gs.ACCEPT, gs.REJECT
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
# the GLV lattice basis of secp256k1 (a_i + b_i lambda = 0 mod N): the split
# leaves k - (nearest lattice point), so its halves fill the parallelogram
# (+-v1 +-v2) / 2 and are largest at its corners
_A1, _B1 = 0x3086D221A7D46BCDE86C90E49284EB15, -0xE4437ED6010E88286F547FA90ABFE4C3
_A2, _B2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8, 0x3086D221A7D46BCDE86C90E49284EB15
assert (_A1 + _B1 * LAMBDA) % N == 0 and (_A2 + _B2 * LAMBDA) % N == 0
SEED = 0xED6E


# ---------------------------------------------------------------------------
# Window geometries (babble_amd/csrc/geometry.h, tests/emu/Makefile) and the
# Python models of the recodings
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Geometry:
    name: str
    W: int        # window bits
    NWIN: int     # windows
    L: int        # sub-table bits: entry d is the chord sum S[d mod 2^L] + S'[d >> L]
    signed: bool  # digits in (-2^(W-1), 2^(W-1)] (else 0 .. 2^W - 1)
    bits: int     # scalar bits the windows cover (256: u1, 128: a GLV half)

    @property
    def top_live(self) -> int:
        """Bits of the top window a scalar of `bits` bits can set."""
        return self.bits - self.W * (self.NWIN - 1)


G26 = Geometry("G26x10", 26, 10, 13, True, 256)   # the product's generator table
G22 = Geometry("G22x12", 22, 12, 11, True, 256)   # tests/emu
G16 = Geometry("G16x17", 16, 17, 8, True, 256)    # the sanitized emulator
K12 = Geometry("K12", 12, 11, 6, True, 128)
K8 = Geometry("K8", 8, 16, 4, False, 128)
KC = Geometry("KC", 22, 6, 11, True, 128)
G_GEOMETRIES = (G26, G22, G16)
K_GEOMETRIES = (K12, K8, KC)
# halves below this bound round-trip through the split with every sign pair
SAFE_HALF_BITS = 126


def signed_digits(u: int, W: int, NWIN: int) -> List[int]:
    """The signed recoding geometry.h describes: u = sum d_j 2^(W j) with every
    d_j in (-2^(W-1), 2^(W-1)].  d_j is the one residue of what is left of u
    mod 2^W in that range; taking it off leaves a multiple of 2^W (a negative
    digit is the carry into the next window)."""
    half, out = 1 << (W - 1), []
    for _ in range(NWIN):
        d = (u + half - 1) % (1 << W) - (half - 1)
        out.append(d)
        u = (u - d) >> W
    assert u == 0, "the top window must absorb the last carry"
    return out


def unsigned_digits(u: int, W: int, NWIN: int) -> List[int]:
    assert u < 1 << (W * NWIN)
    return [(u >> (W * j)) & ((1 << W) - 1) for j in range(NWIN)]


def naf(k: int) -> List[int]:
    """Non-adjacent form, least significant digit first, digits in {-1, 0, 1}."""
    out = []
    while k:
        d = 0
        if k & 1:
            d = 2 - (k & 3)
            k -= d
        out.append(d)
        k >>= 1
    return out


# Digit classes.  For a signed window: t = (the window's W bits of the scalar)
# + (the carry out of the window below) is the value before negation; the
# table slot read is t for t <= 2^(W-1), else 2^W - t with y negated.
SIGNED_CLASSES = ("zero", "one", "sub-1", "sub", "sub+1", "m*sub", "below-sub", "half-1", "half", "half+1",
                  "full", "full+carry")
UNSIGNED_CLASSES = ("zero", "one", "sub-1", "sub", "sub+1", "m*sub", "full")
# the order the classes take along the windows of one scalar: "full" follows
# a class without a carry out, "full+carry" follows "full", and a class that
# leaves a carry is followed by one whose t is at least 1
_SIGNED_CYCLE = ("zero", "sub-1", "sub", "sub+1", "m*sub", "below-sub", "half-1", "half", "full", "full+carry",
                 "half+1", "one")


def window_classes(g: Geometry, u: int) -> List[set]:
    """Per window of scalar u under geometry g: the set of classes its digit
    is in (from the scalar's own bits and the model recoding)."""
    W, L = g.W, g.L
    sub, half, full = 1 << L, 1 << (W - 1), (1 << W) - 1
    raws = [(u >> (W * j)) & full for j in range(g.NWIN)]
    out = []
    if not g.signed:
        for d in unsigned_digits(u, W, g.NWIN):
            c = set()
            for name, hit in (("zero", d == 0), ("one", d == 1), ("sub-1", d == sub - 1), ("sub", d == sub),
                              ("sub+1", d == sub + 1), ("m*sub", d >= 2 * sub and d % sub == 0), ("full", d == full)):
                if hit:
                    c.add(name)
            out.append(c)
        return out
    digits = signed_digits(u, W, g.NWIN)
    cin = 0
    for raw, d in zip(raws, digits):
        t = raw + cin
        assert d == (t if t <= half else t - (1 << W))
        c = set()
        for name, hit in (("zero", t == 0), ("one", t == 1), ("sub-1", t == sub - 1), ("sub", t == sub),
                          ("sub+1", t == sub + 1), ("m*sub", 2 * sub <= t < half and t % sub == 0),
                          ("below-sub", 1 < t < sub - 1), ("half-1", t == half - 1), ("half", t == half),
                          ("half+1", t == half + 1), ("full", raw == full and cin == 0),
                          ("full+carry", raw == full and cin == 1)):
            if hit:
                c.add(name)
        out.append(c)
        cin = 1 if t > half else 0
    return out


def class_value(g: Geometry, cls: str) -> int:
    """The smallest value of a window's own bits that puts it in the class
    without help from a carry.  A top window that cannot hold this value
    cannot be asked for the class."""
    sub, half, full = 1 << g.L, 1 << (g.W - 1), (1 << g.W) - 1
    return {"zero": 0, "one": 1, "sub-1": sub - 1, "sub": sub, "sub+1": sub + 1, "m*sub": 2 * sub, "below-sub": 2,
            "half-1": half - 1, "half": half, "half+1": half + 1, "full": full, "full+carry": full}[cls]


def pack(g: Geometry, v: int, rng: random.Random, top_live: Optional[int] = None,
         force: Optional[Dict[int, str]] = None) -> int:
    """One class in every window of a scalar: window j takes class number
    (j + v) of the cycle, so `len(cycle)` scalars put every class in every
    window (a Latin square).  The top window only takes values below
    2^top_live; a class that does not fit there is replaced by a small one.
    `force`: {window: class} overrides."""
    W, L = g.W, g.L
    sub, half, full = 1 << L, 1 << (W - 1), (1 << W) - 1
    cyc = _SIGNED_CYCLE if g.signed else UNSIGNED_CLASSES
    top_live = g.top_live if top_live is None else top_live
    u, cin = 0, 0
    for j in range(g.NWIN):
        cls = (force or {}).get(j, cyc[(j + v) % len(cyc)])
        live = W if j < g.NWIN - 1 else top_live
        m_end = min(half if g.signed else full + 1, 1 << live) // sub  # m sub below the half and the live bits
        t = {"zero": 0, "one": 1, "sub-1": sub - 1, "sub": sub, "sub+1": sub + 1,
             "m*sub": sub * rng.randrange(2, max(3, m_end)),
             "below-sub": rng.randrange(2, sub - 1), "half-1": half - 1, "half": half, "half+1": half + 1,
             "full": full + cin, "full+carry": full + cin}[cls]
        if force and j in force and cls == "m*sub":
            t = 2 * sub
        raw = max(t - cin, 0) if g.signed else t
        if raw >= 1 << live:
            raw = rng.randrange(2, 1 << min(live, L)) if live >= 2 else 0
        u |= raw << (W * j)
        cin = 1 if g.signed and raw + cin > half else 0
    return u


# ---------------------------------------------------------------------------
# The recovery
# ---------------------------------------------------------------------------
def lift_x(x: int) -> Optional[Tuple[int, int]]:
    """A curve point with this x (x < p), or None: p = 3 mod 4, so a square
    root of c is c^((p+1)/4)."""
    if not 0 <= x < P:
        return None
    c = (x * x * x + 7) % P
    y = pow(c, (P + 1) // 4, P)
    return (x, y) if y * y % P == c else None


def _neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def _digest_int(body: bytes) -> int:
    return int.from_bytes(hashlib.sha256(body).digest(), "big")


def craft(u1: int, u2: Optional[int], tag: str, wrap: bool = False, r: Optional[int] = None,
          x: Optional[int] = None):
    """(body, pubkey65, r, s) of a signature whose verification forms exactly
    u1 G + u2 Q.  With `r` (then u2 is None and comes out as r / s) the point R
    is the lift of `x`, by default r, or r + N with `wrap`: whether x(R) mod N
    equals r is the caller's choice.  Deterministic: the body is the tag and a
    counter."""
    assert 0 < u1 < N and (u2 is None) != (r is None)
    u1g = gs.scalar_mult(u1, gs.G)
    for ctr in range(256):
        body = b"edge-vector|" + tag.encode() + b"|%d\n" % ctr
        e = _digest_int(body) % N
        if e == 0:
            continue
        s = e * pow(u1, -1, N) % N
        rr = u2 * s % N if r is None else r
        k2 = u2 if r is None else rr * pow(s, -1, N) % N
        if rr == 0 or k2 == 0:
            continue
        R = lift_x(rr + N if wrap else rr) if x is None else lift_x(x)
        if R is None:
            if r is not None:
                raise ValueError(f"{tag}: x is not on the curve")
            continue
        if e & 1:
            R = _neg(R)
        T = gs.point_add(R, _neg(u1g))
        if T is None:
            continue
        Q = gs.scalar_mult(pow(k2, -1, N), T)
        return body, gs.Marshal(Q), rr, s
    raise ValueError(f"{tag}: no liftable r in 256 tries")


@dataclass
class Vector:
    tag: str
    body: bytes
    pub: bytes
    r: int
    s: int
    expect: int                     # the status fixed by the construction
    meta: dict = field(default_factory=dict)

    @property
    def family(self) -> str:
        return self.tag[0]

    @property
    def e(self) -> int:
        return _digest_int(self.body)

    @property
    def u1(self) -> int:
        return self.e * pow(self.s, -1, N) % N

    @property
    def u2(self) -> int:
        return self.r * pow(self.s, -1, N) % N


def total_point(v: Vector):
    """u1 G + u2 Q in Python integers (None: the identity)."""
    q = gs.Unmarshal(v.pub)
    assert q is not None
    return gs.point_add(gs.scalar_mult(v.u1, gs.G), gs.scalar_mult(v.u2, q))


def direct_status(v: Vector) -> int:
    """ecdsa.Verify's arithmetic done directly: u1 G + u2 Q, reject the
    identity, reduce x mod N and compare with r."""
    assert 0 < v.r < N and 0 < v.s < N
    R = total_point(v)
    if R is None:
        return REJECT
    return ACCEPT if R[0] % N == v.r else REJECT


# round(2^384 b2 / N) and round(2^384 (-b1) / N): field.h GLV_G1 / GLV_G2
_G1 = 0x3086D221A7D46BCDE86C90E49284EB153DAA8A1471E8CA7FE893209A45DBB031
_G2 = 0xE4437ED6010E88286F547FA90ABFE4C4221208AC9DF506C61571B4AE8AC47F71
assert _G1 == ((_B2 << 384) + N // 2) // N and _G2 == ((-_B1 << 384) + N // 2) // N


def glv_halves(u2: int) -> Tuple[int, int]:
    """(k1, k2), signed, as field.h's glv_split forms them, in Python
    integers: c_i = round(u2 g_i / 2^384), k2 = -c1 b1 - c2 b2,
    k1 = u2 - k2 lambda (mod N), each taken negative above (N - 1) / 2.
    tests/test_edge_vectors.py holds this equal to the product's own split
    (its CPU build, emu_glv_split) on every vector and every dropped pattern."""
    c1, c2 = (u2 * _G1 + (1 << 383)) >> 384, (u2 * _G2 + (1 << 383)) >> 384
    r2 = (c1 * -_B1 + c2 * -_B2) % N
    r1 = (u2 - r2 * LAMBDA) % N
    return (r1 - N if r1 > (N - 1) // 2 else r1), (r2 - N if r2 > (N - 1) // 2 else r2)


# ---------------------------------------------------------------------------
# The set
# ---------------------------------------------------------------------------
class _Builder:
    def __init__(self):
        self.rng = random.Random(SEED)
        self.out: List[Vector] = []
        self.dropped: List[Tuple[str, int, int]] = []  # (tag, k1, k2) the split does not return

    def rand_scalar(self) -> int:
        return self.rng.randrange(1, N)

    def add(self, tag: str, u1: int, u2: int, **meta) -> None:
        body, pub, r, s = craft(u1, u2, tag)
        self.out.append(Vector(tag, body, pub, r, s, ACCEPT, meta))

    def add_halves(self, tag: str, k1: int, k2: int, **meta) -> bool:
        """u2 = k1 + k2 lambda, kept only if the split returns exactly these
        halves and signs."""
        u2 = (k1 + k2 * LAMBDA) % N
        if u2 == 0 or glv_halves(u2) != (k1, k2):
            self.dropped.append((tag, k1, k2))
            return False
        self.add(tag, self.rand_scalar(), u2, k=(k1, k2), **meta)
        return True

    # (a) ------------------------------------------------------------------
    def family_a(self) -> None:
        rng = self.rng
        for g in G_GEOMETRIES:
            W, NWIN = g.W, g.NWIN
            for v in range(len(_SIGNED_CYCLE)):
                self.add(f"a/{g.name}/rot{v}", pack(g, v, rng), self.rand_scalar())
            for j in range(1, NWIN):  # carry chains: every window below bit W j is 2^W - 1; and the carry alone
                k = W * j
                if k < 256:
                    self.add(f"a/{g.name}/2^{k}-1", (1 << k) - 1, self.rand_scalar())
                    self.add(f"a/{g.name}/2^{k}", 1 << k, self.rand_scalar())
            # FROM_INF: window 1 meets the identity, window 0's affine entry, or both
            hi = rng.getrandbits(250 - 2 * W) << (2 * W)
            w0, w1 = rng.randrange(2, 1 << (W - 1)), rng.randrange(2, 1 << (W - 1))
            self.add(f"a/{g.name}/w0=0,w1!=0", hi | w1 << W, self.rand_scalar())
            self.add(f"a/{g.name}/w0!=0,w1=0", hi | w0, self.rand_scalar())
            self.add(f"a/{g.name}/w0=0,w1=0", hi | 1 << (2 * W), self.rand_scalar())
            for j in range(NWIN):  # exactly one non-zero window
                live = W - 1 if j < NWIN - 1 else g.top_live - 1
                if live >= 2:
                    self.add(f"a/{g.name}/only-w{j}", rng.randrange(2, 1 << live) << (W * j), self.rand_scalar())
        for name, u1 in (("1", 1), ("2", 2), ("N-1", N - 1), ("N-2", N - 2)):
            self.add(f"a/u1={name}", u1, self.rand_scalar())

    # (b) ------------------------------------------------------------------
    def family_b(self) -> None:
        rng = self.rng
        for g in K_GEOMETRIES:
            ncls = len(_SIGNED_CYCLE if g.signed else UNSIGNED_CLASSES)
            safe = SAFE_HALF_BITS - g.W * (g.NWIN - 1)
            for v in range(ncls):
                # KC tables are 805 MB a key on the device: one sign pair per
                # rotation there (all four over the rotations), four elsewhere
                pairs = [v % 4] if g is KC else range(4)
                for sp in pairs:
                    k1, k2 = pack(g, v, rng, safe), pack(g, v + 5, rng, safe)
                    s1, s2 = (-1 if sp & 1 else 1), (-1 if sp & 2 else 1)
                    self.add_halves(f"b/{g.name}/rot{v}/{'+-'[sp & 1]}{'+-'[sp >> 1]}", s1 * k1, s2 * k2, geom=g.name)
            # top-window classes above the round-trip bound: kept when the split returns them
            classes = SIGNED_CLASSES if g.signed else UNSIGNED_CLASSES
            for cls in classes:
                if (1 << safe) <= class_value(g, cls) < (1 << g.top_live):
                    for h in (0, 1):
                        # the other half: a patterned one, a short one, and (k2 near 2^127 exists
                        # only beside k1 = -a1 / 2 + 0.29 a2 ~ 0x3760 2^112, same sign) that one
                        others = [pack(g, 3 + 5 * h, rng, safe - 2), rng.getrandbits(64),
                                  (0x3760 << 112) | rng.getrandbits(100)]
                        k = pack(g, 1, rng, g.top_live, force={g.NWIN - 1: cls})
                        tag = f"b/{g.name}/top-{cls}/k{h + 1}"
                        for o in others:
                            pair = (o, k) if h else (k, o)
                            if glv_halves((pair[0] + pair[1] * LAMBDA) % N) == pair:
                                self.add_halves(tag, pair[0], pair[1], geom=g.name)
                                break
                        else:
                            self.dropped.append((tag, 0 if h else k, k if h else 0))
            a, b = pack(g, 2, rng, safe), pack(g, 9, rng, safe)
            self.add_halves(f"b/{g.name}/k1=0", 0, b, geom=g.name)
            self.add_halves(f"b/{g.name}/k2=0", -a, 0, geom=g.name)
            self.add_halves(f"b/{g.name}/k1=k2", a, a, geom=g.name)
            self.add_halves(f"b/{g.name}/k1=-k2", b, -b, geom=g.name)
            for h in (0, 1):  # from-identity shapes of window 0 / window 1 of each half
                hi = rng.getrandbits(120 - 2 * g.W) << (2 * g.W)
                w0, w1 = rng.randrange(2, 1 << (g.W - 1)), rng.randrange(2, 1 << (g.W - 1))
                for name, k in (("w0=0,w1!=0", hi | w1 << g.W), ("w0!=0,w1=0", hi | w0), ("w0=0,w1=0", hi)):
                    ks = [pack(g, 4 + h, rng, safe), pack(g, 6 + h, rng, safe)]
                    ks[h] = k
                    self.add_halves(f"b/{g.name}/k{h + 1}:{name}", ks[0], ks[1] if h else -ks[1], geom=g.name)
        # the largest magnitudes the split returns: just inside the corners
        # (+-v1 +-v2) / 2 of its parallelogram, and the single halves 2^127 - 1, 2^127
        for ci, (c1, c2) in enumerate((((_A1 + _A2) // 2, (_B1 + _B2) // 2), ((_A1 - _A2) // 2, (_B1 - _B2) // 2))):
            for sgn in (1, -1):
                for sh in (8, 24):
                    k1, k2 = sgn * (abs(c1) - (abs(c1) >> sh)) * (1 if c1 > 0 else -1), \
                        sgn * (abs(c2) - (abs(c2) >> sh)) * (1 if c2 > 0 else -1)
                    self.add_halves(f"b/max/corner{ci}{'+-'[sgn < 0]}/2^-{sh}", k1, k2)
        for k in ((1 << 127) - 1, 1 << 127):
            self.add_halves(f"b/max/k1={k:#x},k2=0", k, 0)
            self.add_halves(f"b/max/k1=0,k2={k:#x}", 0, k)

    # (c) ------------------------------------------------------------------
    def family_c(self) -> None:
        dense = int("01" * 63, 2)         # NAF digit +1 at every even bit up to 124: the densest NAF
        dense2 = dense << 1
        burst = int("01" * 19, 2)         # 19 digits, all below bit 37 (k_small's pre-published entries)
        pats = [("dense/dense<<1", dense, dense2), ("dense<<1/dense", dense2, dense), ("dense/empty", dense, 0),
                ("empty/dense", 0, dense), ("burst/empty", burst, 0), ("empty/burst", 0, burst),
                ("burst/burst", burst, burst), ("burst/dense", burst, dense), ("dense/burst", dense, burst)]
        for b in (0, 36, 37, 126, 127):
            pats += [(f"2^{b}/empty", 1 << b, 0), (f"empty/2^{b}", 0, 1 << b)]
        pats += [("2^126/dense", 1 << 126, dense), ("dense/2^126", dense, 1 << 126)]
        for k in (37, 38, 100, 126):
            pats += [(f"2^{k}-1/dense", (1 << k) - 1, dense), (f"dense/2^{k}-1", dense, (1 << k) - 1)]
        pats += [("2^127-1/empty", (1 << 127) - 1, 0)]
        for i, (name, k1, k2) in enumerate(pats):
            self.add_halves(f"c/{name}/{'+-'[i & 1]}{'+-'[(i >> 1) & 1]}", -k1 if i & 1 else k1,
                            -k2 if i & 2 else k2)

    # (d) ------------------------------------------------------------------
    def add_r(self, tag: str, r: int, x: int, expect: int, **meta) -> Vector:
        rng = random.Random(tag)
        body, pub, r, s = craft(rng.randrange(1, N), None, tag, r=r, x=x)
        v = Vector(tag, body, pub, r, s, expect, dict(meta, x=x))
        self.out.append(v)
        return v

    @staticmethod
    def liftable(x: int, step: int) -> int:
        while lift_x(x) is None:
            x += step
        return x

    def family_d(self) -> None:
        rng, up = self.rng, self.liftable
        wraps = []
        x = up(N + rng.randrange(1, P - N), 1)  # x(R) = r + N >= N, r < p - N: the (r + N) branch accepts
        wraps.append(self.add_r("d/wrap/random", x - N, x, ACCEPT, kind="wrap"))
        x = up(P - 1, -1)
        wraps.append(self.add_r("d/wrap/largest-x", x - N, x, ACCEPT, kind="wrap"))
        x = up(N + 1, 1)
        wraps.append(self.add_r("d/wrap/smallest-x", x - N, x, ACCEPT, kind="wrap"))
        r = P - N - 1  # the last r the guard lets through, as x(R) = r and as x(R) = r + N
        while lift_x(r) is None or lift_x(r + N) is None:
            r -= 1
        self.add_r("d/below-p-N/x=r", r, r, ACCEPT, kind="plain")
        wraps.append(self.add_r("d/below-p-N/x=r+N", r, r + N, ACCEPT, kind="wrap"))
        r = up(P - N, 1)  # r at and above p - N with x(R) = r: accepted by the first comparison
        self.add_r("d/at-p-N/x=r", r, r, ACCEPT, kind="plain")
        self.add_r("d/above-p-N/x=r", up(r + 1, 1), up(r + 1, 1), ACCEPT, kind="plain")
        # guard vectors, p - N <= r < N and x(R) = r + N - p: x(R) mod N != r, REJECT.  A
        # check without the r < p - N guard forms r + N in 256 bits: for
        # r + N < 2^256 that is a weakly reduced r + N - p = x(R) (a false
        # ACCEPT); above, the sum wraps to r + N - 2^256, so that x is offered too
        for i, x in enumerate((up(1, 1), up((1 << 256) - P - 1, -1))):
            self.add_r(f"d/guard/x=r+N-p/small{i}", x + P - N, x, REJECT, kind="guard")
        x = up(rng.randrange(1 << 200, 2 * N - P), 1)
        self.add_r("d/guard/x=r+N-p/random", x + P - N, x, REJECT, kind="guard")
        for i, x in enumerate((up(0, 1), up(rng.randrange(1, 2 * N - (1 << 256)), 1))):
            self.add_r(f"d/guard/x=r+N-2^256/{i}", x + (1 << 256) - N, x, REJECT, kind="guard256")
        for w in wraps:  # each accepted wrap vector with r or s flipped in one bit
            for what, bit in (("r", rng.randrange(0, 100)), ("s", rng.randrange(0, 250))):
                r2, s2 = (w.r ^ (1 << bit), w.s) if what == "r" else (w.r, w.s ^ (1 << bit))
                if 0 < r2 < N and 0 < s2 < N:
                    self.out.append(Vector(f"{w.tag}/flip-{what}{bit}", w.body, w.pub, r2, s2, REJECT,
                                           dict(kind="flip")))

    # (e) ------------------------------------------------------------------
    def family_e(self) -> None:
        rng = self.rng
        for i in range(1):
            # u1 G = u2 Q and a valid signature: R = 2 u1 G, r = x(R) mod N, Q = (u1 / u2) G
            tag = f"e/double/accept{i}"
            u1 = self.rand_scalar()
            u1g = gs.scalar_mult(u1, gs.G)
            R = gs.point_add(u1g, u1g)
            r = R[0] % N
            body = b"edge-vector|" + tag.encode() + b"\n"
            s = _digest_int(body) % N * pow(u1, -1, N) % N
            Q = gs.scalar_mult(pow(r * pow(s, -1, N) % N, -1, N), u1g)
            self.out.append(Vector(tag, body, gs.Marshal(Q), r, s, ACCEPT, dict(kind="double")))
            # u1 G = -u2 Q: the total is the identity whatever r says
            tag = f"e/infinity/reject{i}"
            u1, r = self.rand_scalar(), self.rand_scalar()
            body = b"edge-vector|" + tag.encode() + b"\n"
            s = _digest_int(body) % N * pow(u1, -1, N) % N
            Q = _neg(gs.scalar_mult(u1 * pow(r * pow(s, -1, N) % N, -1, N) % N, gs.G))
            self.out.append(Vector(tag, body, gs.Marshal(Q), r, s, REJECT, dict(kind="infinity")))
        # the same totals with Q = G and Q = -G: u1 = +-u2, so r = +-e (mod N);
        # a doubling total there is 2 u1 G with an x that has nothing to do with r
        for qname, Q in (("G", gs.G), ("-G", _neg(gs.G))):
            for sign, kind in ((1, "double" if qname == "G" else "infinity"),
                               (-1, "infinity" if qname == "G" else "double")):
                tag = f"e/{kind}/Q={qname}"
                body = b"edge-vector|" + tag.encode() + b"\n"
                r = sign * _digest_int(body) % N
                self.out.append(Vector(tag, body, gs.Marshal(Q), r, rng.randrange(1, N), REJECT, dict(kind=kind)))


_CACHE: Optional[_Builder] = None


def generate() -> _Builder:
    """The whole set, generated afresh (seeded: the same every time)."""
    b = _Builder()
    b.family_a()
    b.family_b()
    b.family_c()
    b.family_d()
    b.family_e()
    assert len({v.tag for v in b.out}) == len(b.out)
    return b


def _built() -> _Builder:
    global _CACHE
    if _CACHE is None:
        _CACHE = generate()
    return _CACHE


def vectors() -> List[Vector]:
    return _built().out


def dropped() -> List[Tuple[str, int, int]]:
    """(tag, k1, k2) of the half patterns the split did not return."""
    return _built().dropped


_STATUS: Optional[np.ndarray] = None


def direct_statuses() -> np.ndarray:
    """direct_status of every vector (computed once)."""
    global _STATUS
    if _STATUS is None:
        _STATUS = np.array([direct_status(v) for v in vectors()], np.uint8)
    return _STATUS


def kc_subset() -> List[int]:
    """Indices of the vectors that go through the key-cache tables on the
    device (805 MB a key): families d and e and the KC-geometry rotations and
    zero / equal halves of family b."""
    out = []
    for i, v in enumerate(vectors()):
        if v.family in "de" or (v.tag.startswith("b/KC/") and ":" not in v.tag and "/top-" not in v.tag):
            out.append(i)
    return out


def batch(idx: Optional[Sequence[int]] = None, repeat: int = 1):
    """PackedBatch of the vectors (all, or those at `idx`): one message per
    vector, keys de-duplicated by bytes (a flipped vector shares its base's
    key).  `repeat` > 1 repeats every item that many times on the same
    message and key."""
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
