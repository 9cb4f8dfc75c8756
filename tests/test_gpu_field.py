"""Device field / scalar primitives (the generated gfx950 inline asm of
babble_amd/csrc/field_asm.h, through tests/fieldcheck/libfieldcheck.so)
checked against Python integers: fe_mul / fe_sqr / fe_add / fe_sub mod p
(weakly reduced: < 2^256 and congruent), sc_mont (a b 2^-256 mod N, < N) and
fe_inv_var.  Operands include limb patterns that drive every rare block of
the programs (fold carry-outs, tails), so the hardware's carry / hazard
behaviour is exercised, not just the generator's interpreter.  Also every
zipped multi-product program in the calling patterns point.h uses (shared
inputs, outputs on inputs) and every point operation of point.h as a unit:
the bodies under __HIP_DEVICE_COMPILE__ that no host build compiles."""
import ctypes
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "fieldcheck", "libfieldcheck.so")
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
M32 = 2**32 - 1
OPS = {"mul": 0, "sqr": 1, "add": 2, "sub": 3, "mont": 4, "inv": 5,
       "zssm0": 6, "zssm1": 7, "zssm2": 8, "zsss0": 9, "zsss1": 10, "zsss2": 11, "cneg": 12}

pytestmark = pytest.mark.gpu


def _lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/fieldcheck/libfieldcheck.so missing: run __graft_entry__.build()")
    import torch  # noqa: F401  (bind the same HIP runtime torch uses, as babble_amd.native does)

    L = ctypes.CDLL(LIB)
    L.fc_run.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.fc_run.restype = ctypes.c_int
    return L


def _pack(xs):
    out = np.zeros((len(xs), 8), dtype=np.uint32)
    for i, x in enumerate(xs):
        for k in range(8):
            out[i, k] = (x >> (32 * k)) & M32
    return out


def _unpack(arr):
    return [sum(int(arr[i, k]) << (32 * k) for k in range(8)) for i in range(arr.shape[0])]


def _run(op, a, b):
    A, B = _pack(a), _pack(b)
    R = np.zeros_like(A)
    rc = _lib().fc_run(OPS[op], len(a), A.ctypes.data, B.ctypes.data, R.ctypes.data)
    assert rc == 0, rc
    return _unpack(R)


def _operands(seed, n):
    rng = random.Random(seed)
    K = 2**32 + 977
    edge = [0, 1, 2, 977, M32, 2**32, P - 1, P, P + 1, 2**256 - 1, 2**256 - 2, 2**256 - K, 2**256 - K - 1,
            2**256 - K + 1, 2**255, 2**255 - 1, 2 * K, N - 1, N, N + 1]
    top = [2**256 - 1 - rng.getrandbits(rng.choice([1, 8, 16, 40, 64, 128, 200])) for _ in range(n // 4)]
    limbs = [sum(rng.choice([0, M32, M32 - 977, M32 - 976, 1, 2**31]) << (32 * i) for i in range(8))
             for _ in range(n // 4)]
    return edge + top + limbs + [rng.getrandbits(256) for _ in range(n)]


def _pairs(n=4000, seed=11):
    xs = _operands(seed, n // 2)
    ys = _operands(seed + 1, n // 2)
    rng = random.Random(seed + 2)
    a = [rng.choice(xs) for _ in range(n)] + xs
    b = [rng.choice(ys) for _ in range(n)] + [rng.choice(ys) for _ in xs]
    return a, b


@pytest.mark.parametrize("op", ["mul", "sqr", "add", "sub"])
def test_field_ops_match_python_ints(op):
    a, b = _pairs()
    if op == "sqr":
        b = a
    r = _run(op, a, b)
    want = {"mul": lambda x, y: x * y, "sqr": lambda x, y: x * x, "add": lambda x, y: x + y,
            "sub": lambda x, y: x - y}[op]
    bad = [(hex(x), hex(y), hex(z)) for x, y, z in zip(a, b, r) if z >= 2**256 or (z - want(x, y)) % P]
    assert not bad, bad[:5]


def test_fold_carry_blocks_are_hit_and_exact():
    """Products whose high limbs are near 2^32 make Y_i = w_i + (2^32+977) w_(i+8)
    carry out of 64 bits (fe_mul's rare mid block) and R_8 wrap (c9)."""
    rng = random.Random(5)
    a, b = [], []
    for _ in range(4096):
        x = 2**256 - 1 - rng.getrandbits(rng.choice([1, 4, 12, 33, 70]))
        y = 2**256 - 1 - rng.getrandbits(rng.choice([1, 4, 12, 33, 70]))
        a.append(x)
        b.append(y)
    for op in ("mul", "sqr"):
        bb = a if op == "sqr" else b
        r = _run(op, a, bb)
        for x, y, z in zip(a, bb, r):
            assert z < 2**256 and (z - x * y) % P == 0, (op, hex(x), hex(y), hex(z))


def test_add_sub_carry_propagation_blocks_are_exact():
    """fe_add / fe_sub apply K = 2^32 + 977 to limbs 0..1 after a wrap and
    propagate the carry through limbs 2..7 in a rare block: operand pairs
    whose wrapped sum / difference has limbs 0..1 within K of 2^64 (and
    limbs 2..7 all ones, which wrap a second time) enter it."""
    rng = random.Random(9)
    K = 2**32 + 977
    a_add, b_add, a_sub, b_sub = [], [], [], []
    for _ in range(4096):
        lo = 2**64 - 1 - rng.randrange(K + 8)             # low 64 bits of the wrapped value
        hi = rng.choice([rng.getrandbits(192), 2**192 - 1, 2**192 - 2, 0])
        w = (hi << 64) | lo                                # the wrapped value, < 2^256
        a = rng.getrandbits(256)
        if w + 2**256 - a < 2**256:                        # a + b = 2^256 + w
            a_add.append(a)
            b_add.append(w + 2**256 - a)
        lo2 = rng.randrange(K + 8)                         # a - b + 2^256 = w2, limbs 0..1 < K
        w2 = (rng.choice([rng.getrandbits(192), 0, 2**192 - 1]) << 64) | lo2
        b = rng.getrandbits(256)
        if b >= 2**256 - w2 and b + w2 - 2**256 < b:       # a = b + w2 - 2^256 >= 0, a < b
            a_sub.append(b + w2 - 2**256)
            b_sub.append(b)
    assert len(a_add) > 1000 and len(a_sub) > 1000
    for op, xs, ys, f in (("add", a_add, b_add, lambda x, y: x + y), ("sub", a_sub, b_sub, lambda x, y: x - y)):
        r = _run(op, xs, ys)
        bad = [(hex(x), hex(y), hex(z)) for x, y, z in zip(xs, ys, r) if z >= 2**256 or (z - f(x, y)) % P]
        assert not bad, (op, bad[:5])


def test_cneg_canon_matches_python_ints():
    """fe_cneg_canon (the signed-digit table lookups' y negation) on
    canonical operands, including limb patterns that borrow past limb 1."""
    rng = random.Random(13)
    xs = [0, 1, P - 1, P - 2, 2**64 - 1, 2**64, 2**64 - 977, 2**32 + 976, 2**32 + 977, 2**32 + 978]
    xs += [(rng.getrandbits(192) << 64) | rng.choice([0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF00000000 | rng.getrandbits(32),
                                                        0xFFFFFFFEFFFFFC2F, rng.getrandbits(64)])
           for _ in range(3000)]
    xs = [x % P for x in xs]
    flags = [rng.getrandbits(1) for _ in xs]
    r = _run("cneg", xs, flags)
    bad = [(hex(x), f, hex(z)) for x, f, z in zip(xs, flags, r)
           if z >= 2**256 or (z - (-x if f else x)) % P or (not f and z != x)]
    assert not bad, bad[:5]


def test_sc_mont_matches_python_ints():
    a, b = _pairs(3000, 21)
    b = [y % N for y in b]
    r = _run("mont", a, b)
    rinv = pow(2**256, -1, N)
    bad = [(hex(x), hex(y), hex(z)) for x, y, z in zip(a, b, r) if z >= N or z != x * y * rinv % N]
    assert not bad, bad[:5]


LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72  # phi's eigenvalue mod N


def test_item_scalars_match_python_ints():
    """verify_core.h's item_scalars on the device, one item per lane, against
    Python integers: u1 = e s^-1 mod N (< N) for the UNREDUCED 256-bit digest
    e — 0 and N (u1 = 0), k N mod 2^256 for small k (the values a reduction
    that wraps would confuse), N +- 1, 2^256 - N - 1, 2^256 - 1 and _operands'
    edge-heavy values — and the GLV halves of u2 = r s^-1 under the sign
    word, +-k1 +- k2 lambda == u2 (mod N) with k1, k2 < 2^129:
    sc_load_be_words, sc_mont and glv_split as the kernels chain them, crossed
    with s in {1, 2, (N - 1) / 2, N - 1, random} and r in {1, N - 1, random}.
    tests/test_glv_int.py compares glv_split with integers in a host build;
    this is the device's."""
    rng = random.Random(77)
    es = _operands(71, 64)  # the edge list, values near 2^256, limb patterns, random
    es += [0, N, N - 1, N + 1, 2**256 - N - 1, 2**256 - 1] + [k * N % 2**256 for k in range(2, 10)]
    cases = []
    for e in es:
        for s in (1, 2, (N - 1) // 2, N - 1, rng.randrange(1, N)):
            for r in (1, N - 1, rng.randrange(1, N)):
                cases.append((e, r, s))
    n = len(cases)
    assert 500 < n < 5000 and n % 256  # more than one block, a ragged last one

    def be(xs):
        return np.frombuffer(b"".join(x.to_bytes(32, "big") for x in xs), dtype=np.uint32).reshape(len(xs), 8).copy()

    D, R = be([c[0] for c in cases]), be([c[1] for c in cases])
    W = _pack_fast([pow(c[2], -1, N) * 2**256 % N for c in cases])
    out = np.zeros((n, 17), np.uint32)
    L = _lib()
    L.fc_scalars.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 4
    L.fc_scalars.restype = ctypes.c_int
    assert L.fc_scalars(n, D.ctypes.data, R.ctypes.data, W.ctypes.data, out.ctypes.data) == 0
    u1s = _unpack(out[:, :8])
    bad = []
    for i, (e, r, s) in enumerate(cases):
        si = pow(s, -1, N)
        k1 = sum(int(out[i, 8 + k]) << (32 * k) for k in range(4))
        k2 = sum(int(out[i, 12 + k]) << (32 * k) for k in range(4))
        signs = int(out[i, 16])
        k1s, k2s = (-k1 if signs & 1 else k1), (-k2 if signs & 2 else k2)
        ok = (u1s[i] == e * si % N and u1s[i] < N and (k1s + k2s * LAMBDA - r * si) % N == 0
              and k1 < 2**129 and k2 < 2**129 and signs < 4)
        if not ok:
            bad.append((hex(e), hex(r), hex(s), hex(u1s[i]), hex(k1), hex(k2), signs))
    assert not bad, (len(bad), bad[:3])
    assert sum(1 for i, (e, _, _) in enumerate(cases) if e % N == 0 and u1s[i] == 0) >= 2 * 15  # e = 0, e = N


def test_fe_inv_var_matches_python_ints():
    a, _ = _pairs(2000, 31)
    a = [x for x in a if x % P]
    r = _run("inv", a, a)
    bad = [(hex(x), hex(z)) for x, z in zip(a, r) if (z * x - 1) % P]
    assert not bad, bad[:5]


@pytest.mark.parametrize("combo", ["zssm", "zsss"])
def test_zipped_programs_match_python_ints(combo):
    """The interleaved multi-product programs of the key-table doubling chain
    (gen_zip: fe_sqr_sqr_mul_zip / fe_sqr_sqr_sqr_zip), every component, on
    operands that also drive each program's rare blocks."""
    a, b = _pairs(3000, 41)
    rng = random.Random(43)
    for _ in range(1500):  # near-2^256 limbs: fold carry-outs in all three programs at once
        a.append(2**256 - 1 - rng.getrandbits(rng.choice([1, 4, 12, 33, 70])))
        b.append(2**256 - 1 - rng.getrandbits(rng.choice([1, 4, 12, 33, 70])))
    want = {"zssm": [lambda x, y: x * x, lambda x, y: y * y, lambda x, y: x * y],
            "zsss": [lambda x, y: x * x, lambda x, y: y * y, lambda x, y: (x ^ y) ** 2]}[combo]
    for k in range(3):
        r = _run(f"{combo}{k}", a, b)
        bad = [(hex(x), hex(y), hex(z)) for x, y, z in zip(a, b, r) if z >= 2**256 or (z - want[k](x, y)) % P]
        assert not bad, (k, bad[:5])


def _ec_add(p1, p2):
    """Affine secp256k1 addition over Python ints (None = identity)."""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2 and (y1 + y2) % P == 0:
        return None
    if p1 == p2:
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def _ec_mul(k, pt):
    acc = None
    for bit in bin(k)[2:]:
        acc = _ec_add(acc, acc)
        if bit == "1":
            acc = _ec_add(acc, pt)
    return acc


@pytest.mark.parametrize("lat", [0, 1], ids=["gexz_add_ge", "gexz_add_ge_lat"])
def test_xyzz_mixed_add_exceptional_cases(lat):
    """the XYZZ mixed addition of the verify kernels (point.h,
    madd-2008-s; the zipped latency variant too) on the device, against
    Python integers, with the accumulator in random projective form (X = x
    z^2, Y = y z^3, ZZ = z^2, ZZZ = z^3): generic sums, P + P (the
    dbl-2008-s-1 doubling branch), P + (-P) (the identity) and the identity
    plus a point.  Results compared as affine points (X / ZZ, Y / ZZZ)."""
    G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
         0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
    rng = random.Random(17 + lat)
    accs, pts, want = [], [], []
    for i in range(256):
        a = _ec_mul(rng.randrange(1, N), G)
        kind = i % 4
        b = a if kind == 1 else ((a[0], P - a[1]) if kind == 2 else _ec_mul(rng.randrange(1, N), G))
        z = rng.randrange(1, P)
        zz, zzz = z * z % P, z * z * z % P
        if kind == 3:
            accs.append([0, 0, 0, 0, 1])
            want.append(b)
        else:
            accs.append([a[0] * zz % P, a[1] * zzz % P, zz, zzz, 0])
            want.append(_ec_add(a, b))
        pts.append(b)
    A = np.zeros((len(accs), 33), np.uint32)
    Q = np.zeros((len(pts), 16), np.uint32)
    for i, (acc, pt) in enumerate(zip(accs, pts)):
        for j in range(4):
            A[i, 8 * j:8 * j + 8] = _pack([acc[j]])[0]
        A[i, 32] = acc[4]
        Q[i, :8], Q[i, 8:] = _pack([pt[0]])[0], _pack([pt[1]])[0]
    R = np.zeros_like(A)
    L = _lib()
    L.fc_xyzz.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.fc_xyzz.restype = ctypes.c_int
    assert L.fc_xyzz(lat, len(accs), A.ctypes.data, Q.ctypes.data, R.ctypes.data) == 0
    for i, w in enumerate(want):
        X, Y, ZZ, ZZZ = (_unpack(R[i:i + 1, 8 * j:8 * j + 8])[0] % P for j in range(4))
        if w is None:
            assert R[i, 32] == 1, (i, "expected the identity")
            continue
        assert R[i, 32] == 0, i
        assert ZZ and pow(ZZ, 3, P) == pow(ZZZ, 2, P), i
        assert (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P) == w, (i, i % 4)


def test_coop_mul_norm_match_python_ints():
    """coop.h's cooperative product and WIDE reduction (one field element
    per 16-lane DPP row, ONE carry resolve each since round 6) on hardware
    against Python integers, over the edge-heavy operands of the per-lane
    tests plus values whose top limbs are all ones (the unresolved folds'
    largest digits and tail()'s rare second fold).  The digit bounds behind
    the single resolve are asserted by tests/test_coop_model.py."""
    rng = random.Random(31)
    a, b = _pairs(n=6000, seed=41)
    tops = [2**256 - 1 - rng.getrandbits(rng.choice([1, 4, 12, 33, 70])) for _ in range(4000)]
    a += tops
    b += [rng.choice(tops) for _ in tops]
    a = [x % 2**256 for x in a]
    b = [x % 2**256 for x in b]
    A, B = _pack(a), _pack(b)
    L = _lib()
    L.fc_coop_ops.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.fc_coop_ops.restype = ctypes.c_int
    want = {0: lambda x, y: x * y, 1: lambda x, y: x - y, 2: lambda x, y: x - 8 * y, 3: lambda x, y: 3 * x}
    for op, f in want.items():
        R = np.zeros_like(A)
        assert L.fc_coop_ops(op, len(a), A.ctypes.data, B.ctypes.data, R.ctypes.data) == 0
        r = _unpack(R)
        bad = [(op, hex(x), hex(y), hex(z)) for x, y, z in zip(a, b, r) if z >= 2**256 or (z - f(x, y)) % P]
        assert not bad, bad[:5]


def test_coop_xyzz_add_and_double():
    """The wave-cooperative XYZZ addition and doubling of k_small's cold
    path (coop.h add_xyzz / dbl_xyzz: one point per wave, the products of a
    level spread over the four DPP rows), against Python integers.  Both
    operands in random projective form; generic sums, P + P (the doubling
    branch), P + (-P) (the identity), the identity plus a point, and points
    with extreme coordinates.  The doubling's fourth product is beta X3
    (phi's x of the result)."""
    G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
         0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
    beta = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
    rng = random.Random(29)

    def proj(pt, z):
        zz, zzz = z * z % P, z * z * z % P
        return [pt[0] * zz % P, pt[1] * zzz % P, zz, zzz, 0]

    accs, pts, want = [], [], []
    extreme = [_ec_mul(N - 1, G), _ec_mul(2, G), G]
    for i in range(192):
        a = extreme[i % 3] if i < 12 else _ec_mul(rng.randrange(1, N), G)
        kind = i % 4
        b = a if kind == 1 else ((a[0], P - a[1]) if kind == 2 else _ec_mul(rng.randrange(1, N), G))
        za = 1 if i % 16 == 0 else rng.randrange(1, P)
        zb = 1 if i % 8 == 0 else (P - 1 if i % 8 == 1 else rng.randrange(1, P))
        accs.append([0, 0, 0, 0, 1] if kind == 3 else proj(a, za))
        want.append(b if kind == 3 else _ec_add(a, b))
        pts.append((b, proj(b, zb)))
    A = np.zeros((len(accs), 33), np.uint32)
    B = np.zeros((len(pts), 33), np.uint32)
    for i, (acc, (_, pb)) in enumerate(zip(accs, pts)):
        for j in range(4):
            A[i, 8 * j:8 * j + 8] = _pack([acc[j]])[0]
            B[i, 8 * j:8 * j + 8] = _pack([pb[j]])[0]
        A[i, 32] = acc[4]
    R = np.zeros((len(accs), 74), np.uint32)
    L = _lib()
    L.fc_coop_xyzz.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.fc_coop_xyzz.restype = ctypes.c_int
    assert L.fc_coop_xyzz(len(accs), A.ctypes.data, B.ctypes.data, R.ctypes.data) == 0

    def affine(o):
        X, Y, ZZ, ZZZ = (_unpack(R[i:i + 1, o + 8 * j:o + 8 * j + 8])[0] % P for j in range(4))
        assert ZZ and pow(ZZ, 3, P) == pow(ZZZ, 2, P), i
        return X, ZZ, (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)

    for i, w in enumerate(want):
        if w is None:
            assert R[i, 32] == 1, (i, "expected the identity")
        else:
            assert R[i, 32] == 0, i
            assert affine(0)[2] == w, (i, i % 4)
        b = pts[i][0]
        X, ZZ, d = affine(33)
        assert d == _ec_add(b, b), i
        BX = _unpack(R[i:i + 1, 66:74])[0] % P
        assert BX == beta * X % P, i


@pytest.mark.parametrize("w,nwin", [(6, 22), (8, 16), (11, 12)], ids=["K12", "K8", "KC"])
def test_coop_base_chain_equals_per_lane(w, nwin):
    """The wave-cooperative base chain (coop.h: field elements in 16-lane DPP
    rows, the doubling's products spread over the rows, carry-lookahead over
    lane masks) equals the per-lane zipped chain (table_bases_one) mod p on
    every base of every key-table geometry, for random points and points
    with extreme limb patterns (x or y near 0 / p), and prints both chain
    latencies (one key, one wave)."""
    G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
         0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
    rng = random.Random(w)
    pts = [_ec_mul(rng.randrange(1, N), G) for _ in range(60)]
    pts += [G, _ec_mul(2, G), _ec_mul(N - 1, G), _ec_mul(3, G)]
    xy = np.zeros((len(pts), 16), np.uint32)
    for i, (x, y) in enumerate(pts):
        xy[i, :8], xy[i, 8:] = _pack([x])[0], _pack([y])[0]
    L = _lib()
    L.fc_bases.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                           ctypes.POINTER(ctypes.c_float)]
    L.fc_bases.restype = ctypes.c_int
    outs, ms = [], []
    for coop in (0, 1):
        out = np.zeros((len(pts), nwin, 24), np.uint32)
        t = ctypes.c_float()
        assert L.fc_bases(coop, len(pts), xy.ctypes.data, out.ctypes.data, w, nwin, ctypes.byref(t)) == 0
        outs.append(out)
        ms.append(t.value)
    for i in range(len(pts)):
        for j in range(nwin):
            a = [_unpack(outs[0][i:i + 1, j, 8 * c:8 * c + 8])[0] % P for c in range(3)]
            b = [_unpack(outs[1][i:i + 1, j, 8 * c:8 * c + 8])[0] % P for c in range(3)]
            assert a == b, (i, j)
    # the chain's first base is the point itself; the last is 2^(w (nwin-1)) P
    X, Y, Z = [_unpack(outs[1][0:1, nwin - 1, 8 * c:8 * c + 8])[0] % P for c in range(3)]
    zi = pow(Z, -1, P)
    assert (X * zi * zi % P, Y * zi * zi * zi % P) == _ec_mul(2 ** (w * (nwin - 1)), pts[0])
    print(f"\nbase chain {w}x{nwin - 1} doublings, {len(pts)} keys: per-lane {ms[0]:.3f} ms, coop {ms[1]:.3f} ms")


def _pack_fast(xs):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype="<u4").reshape(len(xs), 8).copy()


def _rot(x, k):
    """x's eight 32-bit limbs rotated up by k places."""
    k *= 32
    return ((x << k) | (x >> (256 - k))) & (2**256 - 1)


# (result -> (operand, operand)) of every program and calling pattern of fc_zip
_ZIP = {
    "mul_mul": (0, [[(0, 1), (2, 3)], [(0, 1), (2, 1)], [(0, 1), (2, 3)], [(0, 1), (2, 3)]]),
    "mul_sqr": (1, [[(0, 1), (2, 2)]]),
    "sqr_sqr": (2, [[(0, 0), (1, 1)]]),
    "mul_mul_mul": (3, [[(0, 1), (2, 3), (4, 5)], [(0, 1), (2, 1), (4, 1)], [(0, 1), (2, 3), (4, 3)],
                        [(0, 1), (2, 3), (1, 5)]]),
    "mul_mul_mul_sqr": (4, [[(0, 1), (2, 3), (4, 5), (6, 6)], [(0, 1), (2, 1), (4, 0), (6, 6)]]),
    "sqr_sqr_mul": (5, [[(0, 0), (1, 1), (1, 2)]]),
    "sqr_sqr_sqr": (6, [[(0, 0), (1, 1), (2, 2)]]),
}
_ZIP_OPS = {}


def _zip_operands():
    """Eight operands a lane: (a, b) of _pairs() and of the near-2^256 values
    of test_zipped_programs_match_python_ints, and six more by fixed maps
    that keep an all-ones-heavy value all-ones-heavy (limb rotations, and the
    complement of an xor), so every component of a program sees a
    rare-block operand in the same lane."""
    if not _ZIP_OPS:
        a, b = _pairs(3000, 41)
        rng = random.Random(43)
        for _ in range(1500):
            a.append(2**256 - 1 - rng.getrandbits(rng.choice([1, 4, 12, 33, 70])))
            b.append(2**256 - 1 - rng.getrandbits(rng.choice([1, 4, 12, 33, 70])))
        a = [x % 2**256 for x in a]
        b = [x % 2**256 for x in b]
        full = 2**256 - 1
        cols = [a, b, [_rot(x, 1) for x in a], [_rot(y, 2) for y in b],
                [full ^ _rot(x, 3) ^ _rot(y, 6) for x, y in zip(a, b)], [_rot(y, 5) for y in b],
                [full ^ x ^ y for x, y in zip(a, b)], [0] * len(a)]
        _ZIP_OPS["cols"] = cols
        _ZIP_OPS["packed"] = np.ascontiguousarray(np.stack([_pack_fast(c) for c in cols], axis=1))
    return _ZIP_OPS["cols"], _ZIP_OPS["packed"]


@pytest.mark.parametrize("prog", sorted(_ZIP))
def test_zipped_point_programs_match_python_ints(prog):
    """Every component of the zipped programs the latency point operations
    are built on (fe_mul_mul / fe_mul_sqr / fe_sqr_sqr / fe_mul_mul_mul /
    fe_mul_mul_mul_sqr _zip_asm; the doubling chain's two programs once more
    in their call-site form), < 2^256 and congruent mod p.  Pattern 0 calls a
    program with distinct registers; the others are point.h's call sites:
      fe_mul_mul:  1 b0 == b1          gej_add_ge_lat (x2 Z1Z1, Z1 Z1Z1), gexz_sum_ge_lat / gexz_add_ge_aff (P PP, x1 PP)
                   2 r0 on b0          gexz_sum_ge_lat (t, R, t, u, y1, PPP)
                   3 r0 on b0, r1 on b1  gej_add_ge_lat (t, R, t, HHH, r.Y, HHH)
      fe_mul_mul_mul:  1 b0 == b1 == b2   gexz_add_ge_lat / gexz_add_lat (P PP, X PP, ZZ PP)
                   2 r0 on b0, b1 == b2   gexz_add_ge_lat / gexz_add_lat (t, R, t, u, S1, PPP, ., W12, PPP)
                   3 b0 == a2          gexz_add_lat (S2, b.Y, r.ZZZ, Z12, r.ZZ, b.ZZ, W12, r.ZZZ, b.ZZZ)
      fe_mul_mul_mul_sqr:  1 b0 == b1, a0 == b2   gej_add_ge_lat (H HH, X HH, Z H, R^2)
      fe_sqr_sqr_mul:  a1 == a2        gej_double_lat (X^2, Y^2, Y Z)
      fe_sqr_sqr_sqr:  r1 on a1        gej_double_lat (C, B, t, t, F, E)
    fe_mul_sqr and fe_sqr_sqr have one call form (distinct registers)."""
    code, pats = _ZIP[prog]
    cols, packed = _zip_operands()
    n = len(cols[0])
    L = _lib()
    L.fc_zip.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.fc_zip.restype = ctypes.c_int
    for pat, comps in enumerate(pats):
        out = np.zeros((n, 4, 8), np.uint32)
        assert L.fc_zip(code, pat, n, packed.ctypes.data, out.ctypes.data) == 0
        for k, (ia, ib) in enumerate(comps):
            r = _unpack(out[:, k, :])
            bad = [(i, hex(cols[ia][i]), hex(cols[ib][i]), hex(z)) for i, z in enumerate(r)
                   if z >= 2**256 or (z - cols[ia][i] * cols[ib][i]) % P]
            assert not bad, (prog, pat, k, len(bad), bad[:3])


GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
_POOL = []


def _pool():
    """Points the cases draw from: G, 2 G, (N - 1) G (extreme coordinates)
    and an arithmetic progression from a random point (one addition each)."""
    if not _POOL:
        G = (GX, GY)
        rng = random.Random(53)
        _POOL.extend([G, _ec_mul(2, G), _ec_mul(N - 1, G)])
        pt, step = _ec_mul(rng.randrange(1, N), G), _ec_mul(rng.randrange(1, N), G)
        for _ in range(253):
            _POOL.append(pt)
            pt = _ec_add(pt, step)
    return _POOL


def _neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


Z_CLASSES = ("one", "p-1", "small", "random")


def _zs(rng, cls):
    """Z = 1, p - 1, small (its ZZ and ZZZ can also be given as v + p) or random."""
    return [1, P - 1, rng.randrange(2, 2**10), rng.randrange(1, P)][cls]


def _lift(v, on):
    """v, or with `on` the non-canonical v + p where that is weakly reduced (< 2^256)."""
    return v + P if on and v + P < 2**256 else v


def _xyzz(pt, z, nc):
    if pt is None:
        return [0, 0, 0, 0, 1]
    zz, zzz = z * z % P, z * z * z % P
    return [_lift(pt[0] * zz % P, nc), _lift(pt[1] * zzz % P, nc), _lift(zz, nc), _lift(zzz, nc), 0]


def _jac(pt, z, nc):
    if pt is None:
        return [0, 0, 0, 0, 1]
    return [_lift(pt[0] * z * z % P, nc), _lift(pt[1] * z * z * z % P, nc), _lift(z, nc), 0, 0]


def _aff(pt, z=None, nc=0):
    return [0, 0, 0, 0, 1] if pt is None else [pt[0], pt[1], 1, 1, 0]


# op -> (code, first operand's form, second operand's form, result's form, kinds, expected)
# kinds: 0 generic, 1 P + P, 2 P + (-P), 3 identity + P, 4 P + identity, 5 identity + identity
_POINT_OPS = {
    "gexz_add": (0, _xyzz, _xyzz, "xyzz", (0, 1, 2, 3, 4, 5)),
    "gexz_add_lat": (1, _xyzz, _xyzz, "xyzz", (0, 1, 2, 3, 4, 5)),
    "gexz_sum_ge_lat": (2, _aff, _aff, "xyzz", (0, 1, 2, 3, 4, 5)),
    "gexz_double": (3, _xyzz, _aff, "xyzz", (1,)),
    "gexz_add_ge_aff<throughput,YALT>": (4, _aff, _aff, "xyzz-neg", (0, 1, 2)),
    "gexz_add_ge_aff<LAT>": (5, _aff, _aff, "xyzz", (0, 1, 2)),
    "gexz_add_ge_aff<throughput>": (6, _aff, _aff, "xyzz", (0, 1, 2)),
    "gexz_add_ge(xz_only)": (7, _xyzz, _aff, "xz", (0, 1, 2, 3)),
    "gexz_add_ge<YALT>": (8, _xyzz, _aff, "xyzz-neg", (0, 1, 2, 3, 4, 5)),
    "gexz_add_ge<YALT>(xz_only)": (9, _xyzz, _aff, "xz", (0, 1, 2, 3, 4, 5)),
    "gej_double": (10, _jac, _aff, "jac", (1,)),
    "gej_double_lat": (11, _jac, _aff, "jac", (1,)),
    "gej_double_lat(in place)": (12, _jac, _aff, "jac", (1,)),
    "gej_add_ge": (13, _jac, _aff, "jac", (0, 1, 2, 3)),
    "gej_add_ge_lat": (14, _jac, _aff, "jac", (0, 1, 2, 3)),
    "gej_add": (15, _jac, _jac, "jac", (0, 1, 2, 3, 4, 5)),
}
POINT_LANES = 768


@pytest.mark.parametrize("op", list(_POINT_OPS))
def test_point_ops_match_python_ints(op):
    """Every point operation of point.h as a unit on the device (the
    __HIP_DEVICE_COMPILE__ bodies no host build compiles), 768 lanes each,
    compared as affine points with _ec_add: generic sums, P + P with the two
    operands in different projective representations (the doubling branch),
    P + (-P) (the identity), and the identity on either side and on both
    sides where the operation takes it.  Operands: G, 2 G and (N - 1) G in
    the first lanes of every kind; Z = 1, p - 1, small and random on each
    projective operand of every kind, in every pairing of the two operands'
    classes (asserted below: the kind and the classes are chosen by
    independent indices); and, for small Z, every
    coordinate that allows it given as v + p — a legal weakly reduced input
    with which fe_is_zero has to see p as well as 0 for the P + P and
    P + (-P) branches to be taken.  XYZZ results must keep ZZ^3 == ZZZ^2;
    the identity flag is compared exactly.

    The alternating-Y forms (YALT, the default build's throughput loops)
    return the OPPOSITE of the sum; a lane that adds nothing (the second
    operand's flag: take == false) negates its point, and an accumulator at
    the identity copies the entry it is handed (the caller pre-negates it).
    With xz_only only X and ZZ of a common-path sum are defined: x alone is
    compared there.  gexz_add_ge_aff is run in the three instantiations a
    default build has: <false, true, true> and <true> from the kernels'
    second window, and the plain <false>."""
    code, fa, fb, form, kinds = _POINT_OPS[op]
    yalt = "YALT" in op and "aff" not in op
    pool = _pool()
    rng = random.Random(1000 + code)
    A, B, want = [], [], []
    seen = set()
    for i in range(POINT_LANES):
        # the case kind cycles fastest; the Z classes of the two operands, the non-canonical form and the
        # extreme points are functions of q alone, so every kind meets every one of them
        kind, q = kinds[i % len(kinds)], i // len(kinds)
        ca, cb, lift = q % 4, (q // 4) % 4, (q // 16) % 2
        a = pool[q % 3] if q < 48 else rng.choice(pool)
        b = a if kind == 1 else (_neg(a) if kind == 2 else rng.choice(pool))
        seen.add((kind, "pt", q % 3 if q < 48 else 3))
        if kind in (3, 5):
            a = None
        if kind in (4, 5):
            b = None
        if a is not None and fa is not _aff:
            seen.add((kind, "za", ca, lift))
        if b is not None and fb is not _aff:
            seen.add((kind, "zb", cb, lift))
        if a is not None and b is not None and fa is not _aff and fb is not _aff:
            seen.add((kind, "zab", ca, cb))
        za, zb = _zs(rng, ca), _zs(rng, cb)
        A.append(fa(a, za, lift))
        if yalt:  # the second operand's flag is "adds nothing"; the entry itself is always a point
            e = b if b is not None else rng.choice(pool)
            B.append(fb(e, zb, lift)[:4] + [1 if b is None else 0])
            want.append(e if a is None and b is not None else _neg(_ec_add(a, b)))
        else:
            B.append(fb(b, zb, lift))
            w = _ec_add(a, b)
            want.append(_neg(w) if form == "xyzz-neg" else w)
    assert sum(w is None for w in want) >= POINT_LANES // 12 or kinds == (1,)
    # every kind has seen G, 2 G, (N - 1) G and pool points, and every Z class (plain and v + p) on each
    # projective operand it has, in every pairing of the two operands' classes
    both = [(c, d) for c in range(4) for d in range(4)]
    for kind in kinds:
        got = {t[1:] for t in seen if t[0] == kind}
        assert {("pt", x) for x in range(4)} <= got, (op, kind)
        if fa is not _aff and kind not in (3, 5):
            assert {("za", c, l) for c, l in both if l < 2} <= got, (op, kind)
        if fb is not _aff and kind not in (4, 5):
            assert {("zb", c, l) for c, l in both if l < 2} <= got, (op, kind)
        if fa is not _aff and fb is not _aff and kind in (0, 1, 2):
            assert {("zab", c, d) for c, d in both} <= got, (op, kind)

    def words(rows):
        m = np.zeros((len(rows), 33), np.uint32)
        for j in range(4):
            m[:, 8 * j:8 * j + 8] = _pack_fast([r[j] for r in rows])
        m[:, 32] = [r[4] for r in rows]
        return m

    MA, MB = words(A), words(B)
    R = np.zeros_like(MA)
    L = _lib()
    L.fc_point.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.fc_point.restype = ctypes.c_int
    assert L.fc_point(code, len(A), MA.ctypes.data, MB.ctypes.data, R.ctypes.data) == 0
    cols = [_unpack(R[:, 8 * j:8 * j + 8]) for j in range(4)]
    for i, w in enumerate(want):
        what = (op, i, kinds[i % len(kinds)])
        raw = [cols[j][i] for j in range(4)]
        assert all(v < 2**256 for v in raw), what
        X, Y, Z2, Z3 = (v % P for v in raw)
        if w is None:
            assert R[i, 32] == 1, (what, "expected the identity")
            continue
        assert R[i, 32] == 0, what
        if form == "jac":
            assert Z2, what
            zi = pow(Z2, -1, P)
            got = (X * zi * zi % P, Y * zi * zi * zi % P)
        elif form == "xz":
            assert Z2, what
            assert X * pow(Z2, -1, P) % P == w[0], what
            continue
        else:
            assert Z2 and pow(Z2, 3, P) == pow(Z3, 2, P), what
            got = (X * pow(Z2, -1, P) % P, Y * pow(Z3, -1, P) % P)
        assert got == w, what
