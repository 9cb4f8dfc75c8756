"""Crafted zero-window vectors for BV_Y_ALT (tests/test_y_alt.py on the CPU,
tests/test_gpu_y_alt.py on the device): VALID signatures whose u1, or one GLV
half of whose u2, has a zero signed digit at chosen windows — a step at which
the lane adds nothing and has to negate its stored Y to keep step with the
alternating state (point.h BV_Y_ALT): at window 0, at an even and at an odd
window, at two consecutive windows and at the last window.

The scalars are chosen (edge_vectors.craft finds the key that makes the
signature verify), so a wrong sign anywhere in the chain turns an ACCEPT into
a REJECT; each of those vectors has a key of its own.  shared_key_vectors
puts the same patterns on two fixed keys, for batches that cannot carry more
keys; those signatures do not verify.
"""
import random

from oracle import gosemantics as gs
from tests import edge_vectors as ev

N = ev.N
KW, KNWIN = 12, 11


def patterns(nwin):
    """{name: windows}: which signed digits are forced to zero."""
    return {"w0": (0,), "even": (2,), "odd": (3,), "pair": (nwin - 3, nwin - 2), "last": (nwin - 1,),
            "w0w1": (0, 1)}


def zeroed(rng, w, nwin, windows, bound):
    """A scalar in (0, bound) whose signed w-bit recoding is zero at `windows`
    (the recoding is unique, so clearing digits of a random scalar's recoding
    gives the recoding of the result) and non-zero at the window before the
    first of them, if there is one."""
    while True:
        d = ev.signed_digits(rng.randrange(1, bound), w, nwin)
        for j in windows:
            d[j] = 0
        v = sum(x << (w * j) for j, x in enumerate(d))
        if not 0 < v < bound:
            continue
        d = ev.signed_digits(v, w, nwin)
        if all(d[j] == 0 for j in windows) and (windows[0] == 0 or d[windows[0] - 1] != 0):
            return v


def vectors(gw, gnwin, kw=KW, knwin=KNWIN):
    """[(tag, body, pub, r, s)], every one an ACCEPT.  (gw, gnwin): the
    generator-table geometry whose u1 digits are chosen (26 x 10 on the
    device, 16 x 17 in the host emulator); (kw, knwin): the key-table
    geometry of the GLV halves (K12; 22 x 6 for the key cache)."""
    rng = random.Random(0xA17 + 64 * gw + kw)
    out = []
    for name, windows in patterns(gnwin).items():
        u1 = zeroed(rng, gw, gnwin, windows, N)
        tag = f"yalt/G{gw}/u1/{name}"
        out.append((tag,) + ev.craft(u1, rng.randrange(1, N), tag))
    for half in (0, 1):
        for name, windows in patterns(knwin).items():
            while True:
                k = [rng.randrange(1, 1 << 125), rng.randrange(1, 1 << 125)]
                k[half] = zeroed(rng, kw, knwin, windows, 1 << 125)
                k = [x if rng.random() < 0.5 else -x for x in k]
                u2 = (k[0] + k[1] * ev.LAMBDA) % N
                if u2 and ev.glv_halves(u2) == (k[0], k[1]):
                    break
            tag = f"yalt/K{kw}/h{half}/{name}"
            out.append((tag,) + ev.craft(rng.randrange(1, N), u2, tag))
    return out


def shared_key_vectors(gw, gnwin, kw=KW, knwin=KNWIN):
    """[(tag, body, pub, r, s)] on the two keys of defer_vectors.vectors (so
    that a batch can carry them without more keys than its K12 rule allows):
    u1 and BOTH halves of u2 have the pattern's zero windows.  With the key
    fixed and both scalars chosen the signatures do not verify; the oracle
    decides them, and the CPU test compares the partial sums."""
    rng = random.Random(0x5A17 + 64 * gw + kw)
    out = []
    for key in range(2):
        c = random.Random(0xC0 + key).randrange(1, N)
        pub = gs.Marshal(gs.scalar_mult(c, gs.G))
        for name in patterns(gnwin):
            u1 = zeroed(rng, gw, gnwin, patterns(gnwin)[name], N)
            while True:
                k = [zeroed(rng, kw, knwin, patterns(knwin)[name], 1 << 125) * rng.choice((1, -1)) for _ in range(2)]
                u2 = (k[0] + k[1] * ev.LAMBDA) % N
                if u2 and ev.glv_halves(u2) == (k[0], k[1]):
                    break
            tag = f"yalt/G{gw}K{kw}/k{key}/{name}"
            for ctr in range(256):
                body = b"y-alt|" + tag.encode() + b"|%d\n" % ctr
                e = ev._digest_int(body) % N
                s = e * pow(u1, -1, N) % N
                r = u2 * s % N
                if e and r and 0 < s <= (N - 1) // 2:
                    break
            else:
                raise ValueError(tag)
            out.append((tag, body, pub, r, s))
    return out


def zero_windows(body, r, s, gw, gnwin, kw=KW, knwin=KNWIN):
    """(zero windows of u1, of k1, of k2) of a signature, as the kernels
    recode them."""
    e = ev._digest_int(body) % N
    w = pow(s, -1, N)
    u1, u2 = e * w % N, r * w % N
    k1, k2 = ev.glv_halves(u2)
    z = lambda v, ww, nw: tuple(j for j, x in enumerate(ev.signed_digits(v, ww, nw)) if x == 0)
    return z(u1, gw, gnwin), z(abs(k1), kw, knwin), z(abs(k2), kw, knwin)
