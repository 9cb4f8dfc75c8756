"""Operand quadruples (a, b, x, y) for fe_mul2add (r = a b + x y mod p), shared
by tests/test_field_mul2add.py (the generator's interpreter and the host form)
and tests/test_gpu_field_mul2add.py (the gfx950 program).  Every operand is
below 2^256 (weakly reduced inputs are allowed); the classes drive each block
of the program:

  random     uniform operands
  weak       all-ones, p - 1, p, 2^256 - 1 and their neighbours, mixed
  limb17     a b + x y >= 2^512: the 17th limb w_16 is set
  recount    limbs within a few units of 2^32: a first product of a column
             carries out of 64 bits (the rare re-count of the product phase)
  ycarry     high limbs of the sum all ones: Y_i = w_i + (2^32 + 977) w_(i+8)
             carries out of 64 bits
  tail       the second fold carries out of limb 2 (x = 1 and y chosen so the
             folded low limbs are all ones); half of them also wrap 2^256
"""
import random

P = 2**256 - 2**32 - 977
K = 2**32 + 977
M32 = 2**32 - 1
TOP = 2**256

WEAK = [TOP - 1, P - 1, P, P + 1, TOP - 2, TOP - K, TOP - K - 1, TOP - K + 1, 0, 1, 2**255, 2**255 - 1, 2 * K]


def _near_top(rng):
    return TOP - 1 - rng.getrandbits(rng.choice([1, 4, 12, 33, 70]))


def _tail_case(rng, wrap):
    """x = 1, y free: the low 256 bits L of a b + y are ours to choose.  With
    H the high part, the folded value is L + K H; L makes its low 96 bits (or
    all 256) ones, so adding K (R_8 + 2^32 R_9) >= K carries out of limb 2
    (and out of limb 7)."""
    for _ in range(64):
        a, b = _near_top(rng), rng.getrandbits(256) | (1 << 255)
        h = (a * b) >> 256
        for hh in (h, h + 1):  # y may carry one more unit into the high part
            low = TOP - 1 if wrap else ((rng.getrandbits(160) << 96) | (2**96 - 1))
            want_l = (low - K * hh) % TOP
            y = (want_l - a * b) % TOP
            if (a * b + y) >> 256 == hh and (a * b + y) % TOP == want_l:
                return a, b, 1, y
    raise AssertionError("no tail case found")


def classes(n, seed=1):
    """{class name: [(a, b, x, y), ...]} with about n quadruples per class."""
    rng = random.Random(seed)
    out = {}
    out["random"] = [tuple(rng.getrandbits(256) for _ in range(4)) for _ in range(n)]
    weak = [(w,) * 4 for w in WEAK]
    weak += [tuple(rng.choice(WEAK + [rng.getrandbits(256)]) for _ in range(4)) for _ in range(n)]
    out["weak"] = weak
    out["limb17"] = [tuple(TOP - 1 - rng.getrandbits(rng.choice([1, 64, 200, 254])) for _ in range(4))
                     for _ in range(n)]
    out["limb17"] = [q for q in out["limb17"] if q[0] * q[1] + q[2] * q[3] >= 2**512] + [(TOP - 1,) * 4]
    out["recount"] = [tuple(sum(rng.choice([M32, M32 - 1, M32 - 977, M32 - rng.getrandbits(3)]) << (32 * i)
                                for i in range(8)) for _ in range(4)) for _ in range(n)]
    # x y < 2^288 adds less than 2^32 to the high half 2^256 - (s + t): its limbs 3..7 stay all ones
    out["ycarry"] = [(TOP - 1 - (rng.getrandbits(70) | 1 << 69), TOP - 1 - (rng.getrandbits(70) | 1 << 69),
                      rng.getrandbits(32), rng.getrandbits(256)) for _ in range(n)]
    out["tail"] = [_tail_case(rng, i % 2 == 1) for i in range(n)]
    return out
