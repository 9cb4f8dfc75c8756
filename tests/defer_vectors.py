"""Crafted exception vectors for BV_DEFER_EXC (tests/test_defer_exc.py on the
CPU, tests/test_gpu_defer_exc.py on the device): signatures whose K12 chain
R_G + k1 Q + k2 phi(Q), in the order k_verify_q adds it, meets the entry it is
about to add (a doubling) or its opposite (the identity, from which the next
window restarts) at a chosen GLV half and window.

The key's scalar c is known (Q = c G) and the digest e is whatever the body
hashes to.  u2 is chosen; the Python model of glv_split (edge_vectors) and the
signed 12-bit recoding give every entry of the chain as a scalar times Q (phi
as lambda).  With A the partial sum before window j of half h and B that
window's entry, u1 = c (+-B - A) makes R_G + A = +-B; then s = e / u1 and
r = u2 s.  The signatures need not be valid: the oracle decides them.
"""
import hashlib
import random

from oracle import gosemantics as gs
from tests import edge_vectors as ev

N = ev.N
KW, KNWIN = 12, 11


def chain(u2, w=KW, nwin=KNWIN, signed=True):
    """[(half, window, scalar)] of the entries k_verify_q adds for u2, in
    order (signed w-bit windows x nwin, or K8's unsigned ones with
    signed=False); zero digits add nothing."""
    out = []
    digits = ev.signed_digits if signed else ev.unsigned_digits
    for h, k in enumerate(ev.glv_halves(u2)):
        for j, d in enumerate(digits(abs(k), w, nwin)):
            if d:
                out.append((h, j, (-d if k < 0 else d) * (1 << (w * j)) * (ev.LAMBDA if h else 1) % N))
    return out


def craft(c, u2, half, window, sign, tag, w=KW, nwin=KNWIN):
    """(body, pub, r, s): the chain of u2 meets sign * entry(half, window)."""
    steps = chain(u2, w, nwin)
    at = [i for i, (h, j, _) in enumerate(steps) if (h, j) == (half, window)]
    assert at, "zero digit at the chosen window"
    a = sum(x for _, _, x in steps[:at[0]]) % N
    u1 = c * (sign * steps[at[0]][2] - a) % N
    assert u1
    pub = gs.Marshal(gs.scalar_mult(c, gs.G))
    for ctr in range(256):
        body = b"defer-exc|" + tag.encode() + b"|%d\n" % ctr
        e = int.from_bytes(hashlib.sha256(body).digest(), "big") % N
        if e == 0:
            continue
        s = e * pow(u1, -1, N) % N
        r = u2 * s % N
        if r and 0 < s <= (N - 1) // 2:
            return body, pub, r, s
    raise ValueError(tag)


def vectors(w=KW, nwin=KNWIN):
    """[(tag, body, pub, r, s)]: both signs x first / middle / last window x
    both GLV halves, on two keys.  The last window of half 1 is the trimmed
    (xz_only) addition.  (w, nwin): the key-table geometry whose chain is met
    (K12 by default; 22 x 6 for the key cache's tables, where the same
    construction holds because k_verify_gq sums u1 G first)."""
    rng = random.Random(0xDEFE + w)
    out = []
    for key in range(2):
        c = random.Random(0xC0 + key).randrange(1, N)  # the same two keys for every geometry
        for half in (0, 1):
            for window in (0, nwin // 2, nwin - 1):
                for sign in (1, -1):
                    while True:
                        u2 = rng.randrange(1, N)
                        if any((h, j) == (half, window) for h, j, _ in chain(u2, w, nwin)):
                            break
                    tag = f"W{w}/k{key}/h{half}/w{window}/{'dbl' if sign > 0 else 'inv'}"
                    out.append((tag,) + craft(c, u2, half, window, sign, tag, w, nwin))
    return out
