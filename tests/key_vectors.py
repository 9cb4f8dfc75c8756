"""Public keys at the field boundary (test infrastructure only; the tests are
tests/test_key_vectors.py on the CPU and tests/test_gpu_key_vectors.py on the
device).

key_decode_point (babble_amd/csrc/verify_core.h) is the device's
elliptic.Unmarshal: length 65, prefix 0x04, x < p, y < p, y^2 = x^3 + 7.  The
field arithmetic is weakly reduced (any value below 2^256 stands for its
residue), so the curve equation alone takes a coordinate in [p, 2^256) for its
residue: only fe_ge_p (field.h) tells (x' + p, y) from the real point (x', y).
The out-of-range keys of synth.adversarial ("x >= p": P + 1) and of
tests/golden/gen_golden.py (y = P) are off the curve mod p as well, so the
curve equation rejects them and the range check is never consulted.  The keys
here are the ones that need it:

  x/<x'>/y<i>        (x', +-y): a real point with a small x'            OK
  x+p/<x'>/y<i>      (x' + p, +-y) < 2^256, on the curve mod p          BAD
  top/...            real points whose x is just below p, or differs
                     from 2^256 - 1 in one limb only                    OK
  y/<y'>/r<j>/lo     (x, y'): a real point with a small y'              OK
  y/<y'>/r<j>/hi     (x, p - y')                                        OK
  y+p/<y'>/r<j>      (x, y' + p) < 2^256, on the curve mod p            BAD
  plain/...          x = p, y = p, all ones, all zero                   BAD

x' + p < 2^256 needs x' <= 2^32 + 976.  y for an x is a^((p + 1) / 4) (p = 3
mod 4); x for a y is a cube root of y^2 - 7: p = 7 mod 9, so a cube a has the
root a^((p + 2) / 9) (checked by cubing) and the other two are its products
with beta and beta^2.  The expected result of every key is computed from
Python integers alone (Key.ok).

No private key is known for these points, so the items come in two kinds:
forged valid triples (forged_items: a digest e, r, s with u1 G + u2 Q = R
chosen through a, b; they need an entry that takes the digest from the test)
and items over real message bodies with an in-range (r, s) that does not
verify (real_items: REJECT under a good key, REF_PANIC under a bad one, so
the status alone shows both decode errors).  layout() packs the latter
without BatchBuilder's key de-duplication, each key at a chosen byte
alignment in key_bytes.
"""
import random

import numpy as np

from oracle import gosemantics as gs

P, N = gs.P, gs.N
P0, P1 = P & 0xFFFFFFFF, (P >> 32) & 0xFFFFFFFF  # field.h's limbs 0 and 1 of p; limbs 2..7 are all ones
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
MAX_TWIN = 2**256 - 1 - P  # 2^32 + 976: the largest residue whose sum with p is below 2^256
assert MAX_TWIN == 2**32 + 976 and P % 4 == 3 and P % 9 == 7 and pow(BETA, 3, P) == 1 and BETA != 1

_CACHE = {}


def limbs(v):
    """the eight 32-bit limbs of v, least significant first (fe::v)"""
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def ys_of(x):
    """both y with y^2 = x^3 + 7 (ascending), or () when x^3 + 7 is no square"""
    a = (pow(x, 3, P) + 7) % P
    y = pow(a, (P + 1) // 4, P)
    if y * y % P != a or y == 0:
        return ()
    return tuple(sorted((y, P - y)))


def xs_of(y):
    """the three x with x^3 = y^2 - 7 (ascending), or () when y^2 - 7 is no cube"""
    a = (y * y - 7) % P
    x = pow(a, (P + 2) // 9, P)
    if pow(x, 3, P) != a or a == 0:
        return ()
    return tuple(sorted((x, x * BETA % P, x * BETA * BETA % P)))


def on_curve_x(start, step, stop=None):
    """the x on the curve from `start` in steps of `step` (up to `stop`), lazily"""
    x = start
    while stop is None or (x <= stop if step > 0 else x >= stop):
        if ys_of(x):
            yield x
        x += step


class Key:
    """One encoding: the integers as they are written into the 65 bytes (x, y
    may be >= p), the class it stands for, and the decode result Unmarshal
    must give, from Python integers."""

    def __init__(self, tag, x, y, klass, twin_of=None):
        self.tag, self.x, self.y, self.klass, self.twin_of = tag, x, y, klass, twin_of
        self.pub = b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big")
        self.ok = x < P and y < P and y * y % P == (x**3 + 7) % P

    @property
    def point(self):
        """the point the weakly reduced arithmetic sees"""
        return (self.x % P, self.y % P)


def small_x_values():
    """On-curve x' for the twins: 1, 2, 3 and the largest below 977 (limb 0
    of x' + p stays at or above P0), the first >= 977 and one in
    [2^32 - 2, 2^32) (limb 0 wraps, limb 1 becomes P1 + 1), the first >= 2^32
    and the largest <= 2^32 + 976 (limb 1 = P1 + 1 from x' itself, limb 0 at
    or above P0 again)."""
    below = [x for x in (1, 2, 3) if ys_of(x)]
    assert below == [1, 2, 3]
    return below + [next(on_curve_x(976, -1)), next(on_curve_x(977, 1)), next(on_curve_x(2**32 - 1, -1)),
                    next(on_curve_x(2**32, 1)), next(on_curve_x(MAX_TWIN, -1))]


def small_y_values():
    """y' with a cube root of y'^2 - 7: the two smallest, the nearest below
    and the two nearest from 2^32 up, the largest <= 2^32 + 976; and which of
    them come with all three roots (the others with the smallest root)."""
    def scan(start, step):
        y = start
        while not xs_of(y):
            y += step
        return y

    lo0 = scan(1, 1)
    lo1 = scan(lo0 + 1, 1)
    w0 = scan(2**32, 1)
    vals = [lo0, lo1, scan(2**32 - 1, -1), w0, scan(w0 + 1, 1), scan(MAX_TWIN, -1)]
    return vals, {lo0, vals[-1]}


def keys():
    """every vector key, in a fixed order"""
    if "keys" in _CACHE:
        return _CACHE["keys"]
    out = []
    for xp in small_x_values():
        for i, y in enumerate(ys_of(xp)):
            out.append(Key(f"x/{xp}/y{i}", xp, y, "small-x"))
            out.append(Key(f"x+p/{xp}/y{i}", xp + P, y, "x-twin", twin_of=out[-1].tag))
    # the top of the range (canonical): one root each
    for n, k in enumerate(on_curve_x(P - 1, -1)):
        out.append(Key(f"top/p-{P - k}", k, ys_of(k)[n & 1], "top-limb0"))  # limb 0 just below P0
        if n == 1:
            break
    x = next(on_curve_x(P - 2**32, -1))  # limb 1 = P1 - 1, limb 0 <= P0
    out.append(Key(f"top/p-2^32-{P - 2**32 - x}", x, ys_of(x)[0], "top-limb1"))
    for i in range(1, 8):
        # limb i = 0xFFFFFFFE (limb 1: 0xFFFFFFFD, below P1), limbs below it all ones but for t: limb 0 above P0,
        # limb 1 (i >= 2) above P1
        x = next(on_curve_x(2**256 - 1 - (2 if i == 1 else 1) * 2**(32 * i), -1))
        t = 2**256 - 1 - (2 if i == 1 else 1) * 2**(32 * i) - x
        out.append(Key(f"top/limb{i}-{t}", x, ys_of(x)[i & 1], f"top-hi{i}"))
    vals, all_roots = small_y_values()
    for yp in vals:
        roots = xs_of(yp)
        for j, x in enumerate(roots if yp in all_roots else roots[:1]):
            out.append(Key(f"y/{yp}/r{j}/lo", x, yp, "small-y"))
            out.append(Key(f"y/{yp}/r{j}/hi", x, P - yp, "small-y-neg"))
            out.append(Key(f"y+p/{yp}/r{j}", x, yp + P, "y-twin", twin_of=out[-2].tag))
    out.append(Key("plain/x=p", P, gs.GY, "plain"))
    out.append(Key("plain/y=p", gs.GX, P, "plain"))
    out.append(Key("plain/ones", 2**256 - 1, 2**256 - 1, "plain"))
    out.append(Key("plain/zero", 0, 0, "plain"))
    assert len({k.tag for k in out}) == len(out) == len({k.pub for k in out})
    _CACHE["keys"] = out
    return out


def by_tag():
    return {k.tag: k for k in keys()}


def twins():
    """[(the OK key, its BAD twin)]: the same point to the weakly reduced
    arithmetic"""
    t = by_tag()
    return [(t[k.twin_of], k) for k in keys() if k.twin_of]


def ge_p_case(v):
    """Which comparison of fe_ge_p decides for a value whose limbs 2..7 are
    all ones: "limb1=P1,limb0>=P0", "limb1>P1,limb0<P0" (limb 0 wrapped in
    the sum with p), "limb1>P1,limb0>=P0" (limb 1 raised by the residue's own
    bit 32), or None for a value below p."""
    v = limbs(v)
    assert all(w == 0xFFFFFFFF for w in v[2:])
    if v[1] == P1:
        return "limb1=P1,limb0>=P0" if v[0] >= P0 else None
    if v[1] < P1:
        return None
    return "limb1>P1,limb0>=P0" if v[0] >= P0 else "limb1>P1,limb0<P0"


def first_limb_below_p(v):
    """the most significant limb in which a canonical v is below p"""
    a, b = limbs(v), limbs(P)
    return max(i for i in range(8) if a[i] != b[i])


# ---------------------------------------------------------------------------
# Forged valid triples (digests supplied by the test)
# ---------------------------------------------------------------------------
class Vec:
    """What the consumers of tests/chain_vectors.Vec read: tag, pub, digest,
    r, s, want."""

    def __init__(self, tag, key, digest, r, s, want):
        self.tag, self.key, self.pub, self.digest, self.r, self.s, self.want = tag, key, key.pub, digest, r, s, want


def forge(point, rng):
    """(e, r, s) that verifies under `point` = Q without its private key:
    R = a G + b Q, r = x(R) mod N, s = r / b, e = a s, so u1 = e / s = a and
    u2 = r / s = b; redrawn until r != 0 and 0 < s <= (N - 1) / 2."""
    while True:
        a, b = rng.randrange(1, N), rng.randrange(1, N)
        R = gs.point_add(gs.scalar_mult(a, gs.G), gs.scalar_mult(b, point))
        if R is None:
            continue
        r = R[0] % N
        s = r * pow(b, -1, N) % N
        if r and 0 < s <= (N - 1) // 2:
            return a * s % N, r, s


def forged_items():
    """For every (OK key, BAD twin): one (e, r, s) valid under the point, as
    four items: under the OK key ACCEPT; under the twin REF_PANIC; under the
    twin with r = N and, separately, s = 0, REJECT (the reference reaches the
    malformed key only after the r / s range checks).  The canonical keys
    without a twin (top/, and the -y forms) get one ACCEPT item each."""
    if "forged" in _CACHE:
        return _CACHE["forged"]
    rng = random.Random(0x4B59)
    out, paired = [], set()
    for good, bad in twins():
        e, r, s = forge(good.point, rng)
        d = e.to_bytes(32, "big")
        out.append(Vec(f"forged/{good.tag}", good, d, r, s, gs.ACCEPT))
        out.append(Vec(f"forged/{bad.tag}", bad, d, r, s, gs.REF_PANIC))
        out.append(Vec(f"forged/{bad.tag}/r=N", bad, d, N, s, gs.REJECT))
        out.append(Vec(f"forged/{bad.tag}/s=0", bad, d, r, 0, gs.REJECT))
        paired.add(good.tag)
    for k in keys():
        if k.ok and k.tag not in paired:
            e, r, s = forge(k.point, rng)
            out.append(Vec(f"forged/{k.tag}", k, e.to_bytes(32, "big"), r, s, gs.ACCEPT))
    _CACHE["forged"] = out
    return out


# ---------------------------------------------------------------------------
# Items over real bodies, and layouts
# ---------------------------------------------------------------------------
def real_items():
    """[(key, body, r, s)], one per vector key: an in-range (r, s), s in the
    lower half, drawn without regard to the body, so it does not verify."""
    if "real" in _CACHE:
        return _CACHE["real"]
    rng = random.Random(0x4B5A)
    out = [(k, b"key-vector|" + k.tag.encode(), rng.randrange(1, N), rng.randrange(1, (N - 1) // 2 + 1))
           for k in keys()]
    _CACHE["real"] = out
    return out


JUNK = (b"", b"\x04", b"\x04\x01", b"\x04\x01\x02")  # the leading key of layout(shift): `shift` bytes


def layout(shift, last=None, order=None):
    """(PackedBatch, tags): real_items packed by hand.  key_bytes starts with
    a junk key of `shift` bytes (0: an empty key; 1..3: too short), then every
    vector key, 65 bytes each with no padding, so vector key k sits at
    key_off & 3 == (shift + k) & 3 and the four shifts put every key at every
    alignment.  One item per key in key order, the junk key's item first
    (REF_PANIC).  `last` (a tag) moves that key to the end of key_bytes, where
    nothing of the batch follows it.  `order`: the vector keys' indices to
    take (default all)."""
    from babble_amd.batch import PackedBatch

    items = list(real_items())
    if order is not None:
        items = [items[i] for i in order]
    if last is not None:
        at = [i for i, it in enumerate(items) if it[0].tag == last]
        assert len(at) == 1
        items.append(items.pop(at[0]))
    rng = random.Random(0x4B5B + shift)
    junk = (None, b"key-vector|junk%d" % shift, rng.randrange(1, N), rng.randrange(1, (N - 1) // 2 + 1))
    pubs = [JUNK[shift]] + [it[0].pub for it in items]
    bodies = [junk[1]] + [it[1] for it in items]
    n = len(pubs)
    key_off = np.zeros(n + 1, np.uint64)
    key_off[1:] = np.cumsum([len(p) for p in pubs], dtype=np.uint64)
    msg_off = np.zeros(n + 1, np.uint64)
    msg_off[1:] = np.cumsum([len(m) for m in bodies], dtype=np.uint64)
    rs = [junk[2:]] + [it[2:] for it in items]
    b = PackedBatch(
        msg_bytes=np.frombuffer(b"".join(bodies), np.uint8).copy(), msg_off=msg_off,
        key_bytes=np.frombuffer(b"".join(pubs), np.uint8).copy(), key_off=key_off,
        item_msg=np.arange(n, dtype=np.uint32), item_key=np.arange(n, dtype=np.uint32),
        r_be=np.frombuffer(b"".join(r.to_bytes(32, "big") for r, _ in rs), np.uint8).reshape(n, 32).copy(),
        s_be=np.frombuffer(b"".join(s.to_bytes(32, "big") for _, s in rs), np.uint8).reshape(n, 32).copy(),
        pre=np.zeros(n, np.uint8))
    return b, [f"junk{shift}"] + [it[0].tag for it in items]


LAST_KEY = "x+p/1/y0"  # the key layouts() puts last in key_bytes: a twin


def layouts():
    """{name: (batch, tags)}: the four alignments and the last-key layout"""
    if "layouts" not in _CACHE:
        out = {f"shift{s}": layout(s) for s in range(4)}
        out["last"] = layout(1, last=LAST_KEY)
        _CACHE["layouts"] = out
    return _CACHE["layouts"]


def expected(b):
    """gosemantics.item_status of every item of a packed batch (pre all zero)"""
    out = np.zeros(b.n_items, np.uint8)
    for i in range(b.n_items):
        out[i] = gs.item_status(b.key(int(b.item_key[i])), gs.SHA256(b.message(int(b.item_msg[i]))), *rs_of(b, i))
    return out


def rs_of(b, i):
    """(r, s) of item i of a packed batch, as integers"""
    return int.from_bytes(b.r_be[i].tobytes(), "big"), int.from_bytes(b.s_be[i].tobytes(), "big")


def sig_text(b, i):
    """keys.EncodeSignature of item i's (r, s)"""
    return gs.EncodeSignature(*rs_of(b, i))
