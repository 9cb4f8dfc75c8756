"""Digest edge values through every verify path (tests/test_digest_vectors.py
on the CPU, tests/test_gpu_digest_vectors.py on the device through
tests/chaincheck).

The verify kernels read the 32-byte digest as an UNREDUCED 256-bit integer e
(Go's hashToInt for a 256-bit curve: no truncation, no reduction) and form
u1 = e / s mod N.  A SHA-256 output is 0 or at or above N with probability
2^-128, and tests/chain_vectors.py always supplies e = u1 s mod N with
u1 != 0, so three states of the kernels are reached by no other vector:

  z/  e = 0 (mod N), so u1 = 0: every generator window digit is zero and the
      accumulator is still the identity when the generator chain ends.  With
      Q = c G and a chosen u2: R = u2 Q, r = x(R) mod N, s = r / u2, under the
      digests 0^32 and N.  All ACCEPT.  u2 = 1 (R = Q: one table entry taken
      by an identity accumulator, then no addition), N - 1, lambda, and a
      127-bit k and k lambda (one GLV half zero: the sum is one half's chain
      from the identity).  s is whatever the construction gives: the low-s
      convention of defer_vectors is no property of verification.
  n/  e >= N.  Plain signatures s = (e0 + r c) / k, r = x(k G) mod N, under
      the digests e0 + N (hi) and e0 (lo): both ACCEPT with the same (r, s).
  t/  limb and byte-order patterns of e (2^256 - 1, 2^256 - 2^32, N +- 1,
      2^255, 1, 2^224 - 1, 2^32 - 1), plain signatures on one key.  ACCEPT.
  g/  a generator half that is empty over a whole wave's range of k_small's
      warm tree: u1 a multiple of 2^(GW 2 kWarmSplit[1]) for KC22 and for
      KC18 (wave 0 sums generator pairs only), and u1 = d 2^(GW (GNWIN - 1)),
      the top window alone.  Made as chain_vectors makes its vectors
      (cv.sign_for; digest = u1 s mod N).  ACCEPT.
  x/  twins that must REJECT: z/rand's and z/one's (r, s) under the digests 1
      and N + 1; the digests 0^32 and N with an (r, s) that is valid under the
      digest 1; each n/<e0>/hi signature under e0 + N - 1; t/2^256-1's under
      2^256 - 2.  A path that handles an identity accumulator loosely ends on
      X = ZZ = 0, which final_check's X == r ZZ takes for ANY r: only a
      REJECT vector can show that.

No message hashes to the digests of z/, n/ and most of t/ (that would take a
preimage), so these vectors need a digests-in entry, as chain_vectors' do.
Each vector has the attributes chain_vectors.batch and the runners of
tests/test_gpu_chain_exceptions.py read; u1 and u2 are the scalars the
kernels recover from (digest, r, s).  Python integers over
oracle.gosemantics, seeded, cached in the module."""
import random

from oracle import gosemantics as gs
from tests import chain_vectors as cv
from tests import edge_vectors as ev

N = cv.N
TOP = 1 << 256
# vectors and, of those, REJECT per family (asserted by tests/test_digest_vectors.py)
COUNTS = {"z": (14, 0), "n": (20, 0), "t": (8, 0), "g": (6, 0), "x": (23, 23)}
N_VECTORS, N_REJECT = 71, 23

_CACHE = {}


class Vec:
    """One vector: what chain_vectors.Vec holds, with the digest supplied
    (any 256-bit e) and want fixed by the construction."""

    def __init__(self, tag, c, r, s, e, want):
        assert 0 <= e < TOP and 0 < r < N and 0 < s < N, tag
        self.tag, self.c, self.r, self.s, self.want = tag, c, r, s, want
        self.pub = gs.Marshal(gs.scalar_mult(c, gs.G))
        self.digest = e.to_bytes(32, "big")
        w = pow(s, -1, N)
        self.u1, self.u2 = e * w % N, r * w % N
        self.total = (self.u1 + self.u2 * c) % N
        self.target, self.sign = None, 0

    @property
    def family(self):
        return self.tag[0]

    @property
    def e(self):
        return int.from_bytes(self.digest, "big")


def keys():
    """the two keys of cv.k_vectors("K12")"""
    out = []
    for v in cv.k_vectors("K12"):
        if v.c not in out:
            out.append(v.c)
    assert len(out) == 2
    return out


def zero_sig(c, u2):
    """(r, s) that verifies under Q = c G exactly when e = 0 (mod N):
    R = u2 Q, r = x(R) mod N, s = r / u2."""
    r = gs.scalar_mult(u2 * c % N, gs.G)[0] % N
    s = r * pow(u2, -1, N) % N
    assert r and s
    return r, s


def plain_sig(c, e, rng):
    """(r, s) of a plain signature over the digest e by the key c:
    r = x(k G) mod N, s = (e + r c) / k, redrawn while r or s is 0."""
    while True:
        k = rng.randrange(1, N)
        r = gs.scalar_mult(k, gs.G)[0] % N
        s = (e + r * c) * pow(k, -1, N) % N
        if r and s:
            return r, s


E0_NAMES = ("1", "2^32", "2^128", "2^256-N-1", "rand")
T_VALUES = (("2^256-1", TOP - 1), ("2^256-2^32", TOP - (1 << 32)), ("N-1", N - 1), ("N+1", N + 1), ("2^255", 1 << 255),
            ("1", 1), ("2^224-1", (1 << 224) - 1), ("2^32-1", (1 << 32) - 1))


def g_shifts():
    """(name, bits) of the g/ family: the generator windows below `bits` are
    wave 0's whole range of the warm tree on KC22 / on KC18 (generator pairs
    only), and the top window alone."""
    split = cv.small_constants()["kWarmSplit"]
    out = []
    for geom in ("KC22", "KC18"):
        assert split[geom][1] <= cv.GNWIN // 2, geom  # wave 0's range holds generator pairs only
        out.append((f"wave0-{geom}", cv.GW * 2 * split[geom][1]))
    return out + [("top-window", cv.GW * (cv.GNWIN - 1))]


def vectors():
    """all families, in the order z, n, t, g, x"""
    if "all" in _CACHE:
        return _CACHE["all"]
    rng = random.Random(0xD16E)
    A, R = gs.ACCEPT, gs.REJECT
    out, twins = [], []
    cs = keys()
    lam = ev.LAMBDA
    e0s = dict(zip(E0_NAMES, (1, 1 << 32, 1 << 128, TOP - N - 1, rng.randrange(1, TOP - N))))
    for kidx, c in enumerate(cs):
        k = f"k{kidx}"
        # z/ -------------------------------------------------------------
        u2 = rng.randrange(2, N - 1)
        zr = zero_sig(c, u2)
        out.append(Vec(f"z/rand/{k}", c, *zr, 0, A))
        out.append(Vec(f"z/N/{k}", c, *zr, N, A))
        zo = zero_sig(c, 1)
        out.append(Vec(f"z/one/{k}", c, *zo, 0, A))
        out.append(Vec(f"z/minus-one/{k}", c, *zero_sig(c, N - 1), N, A))
        out.append(Vec(f"z/lambda/{k}", c, *zero_sig(c, lam), 0, A))
        kk = rng.getrandbits(126) | 1 << 126
        out.append(Vec(f"z/half0/{k}", c, *zero_sig(c, kk), N, A))
        out.append(Vec(f"z/half1/{k}", c, *zero_sig(c, kk * lam % N), 0, A))
        for name, sig in (("z-rand", zr), ("z-one", zo)):
            twins.append(Vec(f"x/{name}/e=1/{k}", c, *sig, 1, R))
            twins.append(Vec(f"x/{name}/e=N+1/{k}", c, *sig, N + 1, R))
        one = plain_sig(c, 1, rng)
        twins.append(Vec(f"x/valid-under-1/e=0/{k}", c, *one, 0, R))
        twins.append(Vec(f"x/valid-under-1/e=N/{k}", c, *one, N, R))
    for kidx, c in enumerate(cs):
        # n/ -------------------------------------------------------------
        for name, e0 in e0s.items():
            assert 0 < e0 < TOP - N
            sig = plain_sig(c, e0, rng)
            out.append(Vec(f"n/{name}/hi/k{kidx}", c, *sig, e0 + N, A))
            out.append(Vec(f"n/{name}/lo/k{kidx}", c, *sig, e0, A))
            twins.append(Vec(f"x/n-{name}-hi/e-1/k{kidx}", c, *sig, e0 + N - 1, R))
    # t/ -----------------------------------------------------------------
    for name, e in T_VALUES:
        sig = plain_sig(cs[0], e, rng)
        out.append(Vec(f"t/{name}", cs[0], *sig, e, A))
        if e == TOP - 1:
            twins.append(Vec("x/t-2^256-1/e-1", cs[0], *sig, TOP - 2, R))
    # g/ -----------------------------------------------------------------
    for kidx, c in enumerate(cs):
        for name, bits in g_shifts():
            while True:
                u1 = rng.randrange(1, 1 << (255 - bits)) << bits  # (the top window: a positive signed digit < 2^21)
                u2 = rng.randrange(1, N)
                rs = cv.sign_for(c, u1, u2)
                if rs and (u1 + u2 * c) % N:
                    break
            v = Vec(f"g/{name}/k{kidx}", c, rs[0], rs[1], u1 * rs[1] % N, A)
            assert (v.u1, v.u2) == (u1, u2)
            out.append(v)
    out += twins
    assert len({v.tag for v in out}) == len(out)
    _CACHE["all"] = out
    return out


def family(f):
    return [v for v in vectors() if v.family == f]
