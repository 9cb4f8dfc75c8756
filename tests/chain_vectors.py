"""VALID signatures whose addition chains meet an exceptional addition
(tests/test_chain_exceptions.py on the CPU, tests/test_gpu_chain_exceptions.py
on the device through tests/chaincheck).

tests/defer_vectors.py makes a chain meet the entry it is about to add under a
real SHA-256 digest, so its signatures are invalid, and a mishandled doubling
or P + (-P) only turns one REJECT into another.  Here the TEST supplies the
digest: with the key Q = c G and chosen u1, u2 (t = u1 + u2 c), R = t G,
r = x(R) mod N, s = r / u2 and e = u1 s, the 32 big-endian bytes of e are a
digest under which (r, s) verifies — the kernels recover exactly u1 = e / s
and u2 = r / s — so a wrong point anywhere in the chain turns an ACCEPT into a
REJECT.  No message hashes to such a digest (that would take a preimage), which
is why these vectors need the digests-in entry of tests/chaincheck.

The conventions of defer_vectors.craft hold: r != 0 and 0 < s <= (N - 1) / 2
(u2 is redrawn until they do).  A vector whose total is the identity (the
last step of a chain met with the opposite sign) has no R; it takes r from a
fixed point and is REJECT.  Everything is cached in the module.

Order models (each chain as a list of (label, scalar) steps; a scalar s stands
for the point s G, so "the accumulator equals the entry or its opposite" is
acc == +-s mod N, exact):
  * K12 / K8 device order, KC22 / KC18 bulk (k_verify_g + k_verify_q,
    k_verify_gq): u1 G whole (the generator chain cannot collide:
    tests/test_defer_exc.py), then the key table's half 0 and half 1, windows
    ascending (defer_vectors.chain; K8 with the unsigned recoding).  Solved
    for u1.
  * generic path (verify_item_generic): u2 Q whole, then the generator's
    26-bit signed windows ascending.  u2 c + A_G = +-B_G is solved for c.
  * host-entry order, every key-table geometry (k_verify_qf, then
    k_verify_gf: bv_item_pipe, which bv_verify_batch, bv_verify_batch_text,
    bv_verify_events* and bv_verify_blocks run): the key chain from the
    identity, half 0 then half 1, then the generator's windows onto R_Q
    (host_steps).  The same equation, solved for u2 with c fixed.
  * k_small without a key table (cold): wave 3 adds the G sum in phase
    kColdGJoin and +-phi(2^i Q) for the NAF digits of k2 ascending, at most
    kColdBudget additions a phase from the entries published so far
    (kColdPre + j kColdChunk); wave 1 the same for k1 without the G sum, then
    the final k1 Q + acc3 (an identity acc3 is skipped).  Solved for u1.
  * k_small with a cached table (warm, KC22 and KC18): 10 G leaves and
    2 KNWIN table leaves, summed in affine pairs, then wave w sums nodes
    [kWarmSplit[w], kWarmSplit[w + 1]), waves 0 and 1 the 4 -> 2 level, wave
    0 the root; identity leaves and nodes are skipped.  The cross-chain
    additions (a G-only sum meeting a key node) are solved for c.
The small-kernel constants are read from kernels.hip (small_constants), so a
retuned schedule changes the model with it.  Neither the generic path nor
k_small has a host build (coop.h is device-only): that their vectors hit
the targeted addition rests on these models, which the CPU test checks in
Python integers — the modelled operands are equal or opposite at the
targeted step and at no other — and on nothing that runs the kernels'
source.  "At no other" reaches as far as each model does: the generic path's
u2 Q is ONE step here (its 128 double-and-add steps on k1 Q + k2 phi(Q) are
not modelled, nor targeted), as is each key chain's u1 G; wave 1's k1 chain
on the cold path, the generator tree and the warm tree's leaf pairs are
modelled (so a collision there would be reported) but never targeted: their
operands differ in magnitude by construction.  The host-record form of
k_small (rec != NULL) runs the same two schedules over the u1, k1, k2 that
bv_host_item_records forms, so the cold and warm vectors serve it as they are.
In the host-entry order the key chain is modelled window by window and the
generator chain likewise; only the generator windows are targeted.
"""
import os
import random
import re

from oracle import gosemantics as gs
from tests import defer_vectors as dv
from tests import edge_vectors as ev

N = ev.N
GW, GNWIN = 26, 10  # geometry.h BV_GW, BV_GNWIN (asserted against the header by tests/test_chain_exceptions.py)
# (window bits, windows, signed) of the key-table chains
K_GEOMETRIES = {"K12": (12, 11, True), "K8": (8, 16, False), "KC22": (22, 6, True), "KC18": (18, 8, True)}
IDENTITY_R = gs.G[0] % N  # r of the vectors whose total is the identity (any r in range: they are REJECT)

_CACHE = {}


class Vec:
    """One vector: pub (65 bytes), digest (32 bytes), r, s, the expected
    status, and what it was made from (c, u1, u2, the targeted step)."""

    def __init__(self, tag, c, u1, u2, r, s, target, sign):
        self.tag, self.c, self.u1, self.u2, self.r, self.s = tag, c, u1, u2, r, s
        self.target, self.sign = target, sign
        self.pub = gs.Marshal(gs.scalar_mult(c, gs.G))
        self.digest = (u1 * s % N).to_bytes(32, "big")
        self.total = (u1 + u2 * c) % N
        self.want = gs.ACCEPT if self.total else gs.REJECT


def sign_for(c, u1, u2):
    """(r, s) of the valid signature with these u1, u2 under Q = c G, or None
    when r == 0 or s is not in (0, (N - 1) / 2]."""
    t = (u1 + u2 * c) % N
    r = gs.scalar_mult(t, gs.G)[0] % N if t else IDENTITY_R
    s = r * pow(u2, -1, N) % N
    if r == 0 or not 0 < s <= (N - 1) // 2:
        return None
    return r, s


def plain(seed, n, c=None):
    """n plain valid vectors made the same way (random u1, u2; no collision
    sought): the filler of the large batches and the negative control."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        cc = c if c is not None else rng.randrange(1, N)
        u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
        rs = sign_for(cc, u1, u2)
        if rs and (u1 + u2 * cc) % N:
            out.append(Vec(f"plain/{seed}/{len(out)}", cc, u1, u2, rs[0], rs[1], None, 0))
    return out


# ---------------------------------------------------------------------------
# Order models
# ---------------------------------------------------------------------------
def k_steps(v_or_u1, u2=None, c=None, geom="K12"):
    """The device-order chain of a key-table path: [(label, scalar)], the
    first step the whole u1 G."""
    if u2 is None:
        v_or_u1, u2, c = v_or_u1.u1, v_or_u1.u2, v_or_u1.c
    w, nwin, signed = K_GEOMETRIES[geom]
    return [("G", v_or_u1 % N)] + [((h, j), x * c % N) for h, j, x in dv.chain(u2, w, nwin, signed)]


def generic_steps(u1, u2, c):
    """verify_item_generic's chain: u2 Q whole, then u1's signed 26-bit
    generator windows ascending (zero digits add nothing)."""
    out = [("Q", u2 * c % N)]
    for j, d in enumerate(ev.signed_digits(u1, GW, GNWIN)):
        if d:
            out.append((("g", j), (d << (GW * j)) % N))
    return out


def host_steps(u1, u2, c, geom):
    """The host-entry order (k_verify_qf, then k_verify_gf): the key chain of
    `geom` from the identity, half 0 then half 1, windows ascending, then
    u1's signed 26-bit generator windows ascending onto R_Q (generic_steps'
    generator steps)."""
    w, nwin, signed = K_GEOMETRIES[geom]
    return [(("k", h, j), x * c % N) for h, j, x in dv.chain(u2, w, nwin, signed)] + generic_steps(u1, u2, c)[1:]


def collisions(steps):
    """[(label, sign)] of the steps at which the accumulator (the sum of the
    steps before, from the identity) equals the step's entry (+1: a
    doubling) or its opposite (-1: the identity).  A zero accumulator takes
    the entry and collides with nothing; a zero entry (an identity node) is
    skipped by the kernels and by this."""
    out, acc = [], 0
    for label, x in steps:
        if not x:
            continue
        if acc:
            if acc == x:
                out.append((label, 1))
            elif (acc + x) % N == 0:
                out.append((label, -1))
        acc = (acc + x) % N
    return out


# ---------------------------------------------------------------------------
# Crafting
# ---------------------------------------------------------------------------
def _targets(labels):
    """first, a middle and the last of the non-zero steps"""
    return sorted({0, len(labels) // 2, len(labels) - 1})


def k_vectors(geom):
    """Both signs x the first, a middle and the last non-zero window of each
    GLV half, on two keys: 24 vectors, the chain of `geom` meeting the
    targeted entry.  (defer_vectors.vectors' targets, made valid.)"""
    key = ("k", geom)
    if key in _CACHE:
        return _CACHE[key]
    w, nwin, signed = K_GEOMETRIES[geom]
    rng = random.Random(0xC4A1 + w)
    out = []
    for kidx in range(2):
        c = random.Random(0xC0 + kidx).randrange(1, N)  # defer_vectors' two keys
        for half in (0, 1):
            for which in range(3):
                for sign in (1, -1):
                    while True:
                        u2 = rng.randrange(1, N)
                        steps = dv.chain(u2, w, nwin, signed)
                        mine = [i for i, (h, _, _) in enumerate(steps) if h == half]
                        if len(mine) < 3:
                            continue
                        at = mine[_targets(mine)[which]]
                        a = sum(x for _, _, x in steps[:at]) % N
                        u1 = c * (sign * steps[at][2] - a) % N
                        rs = sign_for(c, u1, u2) if u1 else None
                        if rs:
                            break
                    h, j, _ = steps[at]
                    tag = f"{geom}/k{kidx}/h{h}/w{j}/{'dbl' if sign > 0 else 'inv'}"
                    out.append(Vec(tag, c, u1, u2, rs[0], rs[1], (h, j), sign))
    _CACHE[key] = out
    return out


def generic_vectors():
    """Both signs x the first, a middle and the last non-zero generator
    window, twice over: 12 vectors, each on a key of its own (the collision
    is solved for c)."""
    if "generic" in _CACHE:
        return _CACHE["generic"]
    rng = random.Random(0x6E7E)
    out = []
    for rep in range(2):
        for which in range(3):
            for sign in (1, -1):
                while True:
                    u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
                    g = generic_steps(u1, u2, 1)[1:]
                    if len(g) < 3:
                        continue
                    at = _targets(g)[which]
                    a = sum(x for _, x in g[:at]) % N
                    c = (sign * g[at][1] - a) * pow(u2, -1, N) % N
                    rs = sign_for(c, u1, u2) if c else None
                    if rs:
                        break
                tag = f"generic/{rep}/g{g[at][0][1]}/{'dbl' if sign > 0 else 'inv'}"
                out.append(Vec(tag, c, u1, u2, rs[0], rs[1], g[at][0], sign))
    _CACHE["generic"] = out
    return out


def host_vectors():
    """The host-entry order, on k_vectors' two keys: R_Q = u2 Q, whole when
    k_verify_gf adds the generator windows onto it, meets the first, a middle
    and the last non-zero generator window of u1 as a doubling and as
    P + (-P): 12 vectors (the 2 that meet the last window's opposite end on
    the identity: REJECT).  u1 is drawn and the collision solved for u2 with
    c fixed, u2 = (+-g_at - sum of the windows below) / c, so every key-table
    geometry runs the same vectors on two key tables; that u2's own key chain
    (from the identity) meets nothing under a geometry is what
    tests/test_chain_exceptions.py checks with host_steps."""
    if "host" in _CACHE:
        return _CACHE["host"]
    rng = random.Random(0x4057)
    out = []
    for kidx in range(2):
        c = random.Random(0xC0 + kidx).randrange(1, N)
        for which in range(3):
            for sign in (1, -1):
                while True:
                    u1 = rng.randrange(1, N)
                    g = generic_steps(u1, 0, 1)[1:]
                    if len(g) < 3:
                        continue
                    at = _targets(g)[which]
                    a = sum(x for _, x in g[:at]) % N
                    u2 = (sign * g[at][1] - a) * pow(c, -1, N) % N
                    rs = sign_for(c, u1, u2) if u2 else None
                    if rs:
                        break
                tag = f"host/k{kidx}/g{g[at][0][1]}/{'dbl' if sign > 0 else 'inv'}"
                out.append(Vec(tag, c, u1, u2, rs[0], rs[1], g[at][0], sign))
    _CACHE["host"] = out
    return out


def host_invalid_twins():
    """host_vectors' chains under signatures that do NOT verify: the same c,
    u1 and u2, so the same additions and the same collision, with another s'
    (drawn), r' = u2 s' and the digest u1 s' — r' is then not x(R), and the
    status is REJECT.  What they are for: an unchecked chain (BV_DEFER_EXC)
    that has met P == 0 ends, one addition later, on X = ZZ = 0, which
    final_check's X == r ZZ takes for ANY r; an item that is flagged and not
    redone therefore ACCEPTs, which a valid signature cannot show.  12."""
    if "host-twins" in _CACHE:
        return _CACHE["host-twins"]
    rng = random.Random(0x7714)
    out = []
    for v in host_vectors():
        x_r = gs.scalar_mult(v.total, gs.G)[0] % N if v.total else None
        while True:
            s = rng.randrange(1, (N - 1) // 2 + 1)
            r = v.u2 * s % N
            if r and r != x_r and s != v.s:
                break
        t = Vec(v.tag.replace("host/", "host-invalid/"), v.c, v.u1, v.u2, r, s, v.target, v.sign)
        t.want = gs.REJECT
        out.append(t)
    _CACHE["host-twins"] = out
    return out


def batch(vecs, repeat=1):
    """(PackedBatch, digests, expected statuses): one message slot (an empty
    body: nothing reads it), one digest and one item per vector, keys shared;
    the whole list repeated `repeat` times as further items."""
    import numpy as np

    from babble_amd.batch import BatchBuilder

    bb = BatchBuilder()
    for v in vecs:
        bb.add_item_raw(bb.add_msg(b"chain|" + v.tag.encode()), bb.add_key(v.pub), 0, v.r.to_bytes(32, "big"),
                        v.s.to_bytes(32, "big"))
    b = bb.pack()
    dig = np.frombuffer(b"".join(v.digest for v in vecs), np.uint8).reshape(len(vecs), 32).copy()
    want = np.array([v.want for v in vecs], np.uint8)
    if repeat > 1:
        from babble_amd.batch import PackedBatch

        b = PackedBatch(msg_bytes=b.msg_bytes, msg_off=b.msg_off, key_bytes=b.key_bytes, key_off=b.key_off,
                        item_msg=np.tile(b.item_msg, repeat), item_key=np.tile(b.item_key, repeat),
                        r_be=np.tile(b.r_be, (repeat, 1)), s_be=np.tile(b.s_be, (repeat, 1)),
                        pre=np.tile(b.pre, repeat) if b.pre is not None else None)
        want = np.tile(want, repeat)
    return b, dig, want


# ---------------------------------------------------------------------------
# k_small: constants from the source, order models, crafting
# ---------------------------------------------------------------------------
KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "babble_amd", "csrc", "kernels.hip")
WARM_GEOMETRIES = {"KC22": (22, 6, "BV_KCNWIN"), "KC18": (18, 8, "BV_KC18NWIN")}


def small_constants():
    """kColdPre, kColdChunk, kColdBudget, kColdGJoin and kWarmSplit (per
    cached geometry) as kernels.hip defines them."""
    if "consts" in _CACHE:
        return _CACHE["consts"]
    src = open(KERNELS).read()

    def num(name):
        m = re.search(r"constexpr uint32_t %s = (\d+);" % name, src)
        assert m, name
        return int(m.group(1))

    m = re.search(r"constexpr uint32_t kColdPre = ([^;]+);", src)
    assert m and m.group(1).strip() == "1 + kColdD0 + kColdD1", m and m.group(1)
    out = {"kColdPre": 1 + num("kColdD0") + num("kColdD1"), "kColdChunk": num("kColdChunk"),
           "kColdBudget": num("kColdBudget"), "kColdGJoin": num("kColdGJoin"), "kWarmSplit": {}}
    for geom, (_, nwin, macro) in WARM_GEOMETRIES.items():
        m = re.search(r"kWarmSplit<%s>\[5\] = \{(\d+), (\d+), (\d+), (\d+), small_warm<%s>::kNodes\}" % (macro, macro), src)
        assert m, geom
        out["kWarmSplit"][geom] = [int(x) for x in m.groups()] + [(GNWIN + 2 * nwin + 1) // 2]
    _CACHE["consts"] = out
    return out


def cold_chains(u1, u2, c):
    """{name: steps} of k_small's cold path: wave 3's chain, and wave 1's
    with the final addition of acc3 at its end."""
    k = small_constants()
    halves = ev.glv_halves(u2)
    nafs = [ev.naf(abs(h)) for h in halves]
    nb = max(len(n) for n in nafs)

    def wave(h):
        steps, pos, digits = [], 0, nafs[h]
        sgn, mult = (-1 if halves[h] < 0 else 1), (ev.LAMBDA if h else 1)
        for j in range(64):
            budget = k["kColdBudget"]
            if h and j == k["kColdGJoin"]:
                steps.append(("G", u1 % N))
                budget -= 1
            end = min(nb, k["kColdPre"] + j * k["kColdChunk"])
            while pos < end:
                if pos < len(digits) and digits[pos]:
                    if budget == 0:
                        break
                    budget -= 1
                    steps.append((("n", pos), sgn * digits[pos] * (1 << pos) * mult * c % N))
                pos += 1
            if pos >= nb and j >= k["kColdGJoin"]:
                break
        assert pos >= nb
        return steps

    w3, w1 = wave(1), wave(0)
    return {"wave3": w3, "wave1": w1 + [("acc3", sum(x for _, x in w3) % N)]}


def all_collisions(chains):
    return sorted((name, label, sign) for name, steps in chains.items() for label, sign in collisions(steps))


def cold_vectors():
    """k_small's cold path, two keys: wave 3's chain meeting the first, a
    middle and the last NAF digit of k2 with both signs (the last with the
    opposite sign leaves acc3 the identity: ACCEPT with R = k1 Q); the final
    k1 Q + acc3 as a doubling (u1 = c (k1 - lambda k2)); acc3 handed over as
    the identity (u1 = -c lambda k2); the identity total (REJECT): 18."""
    if "cold" in _CACHE:
        return _CACHE["cold"]
    rng = random.Random(0xC01D)
    out = []
    for kidx in range(2):
        c = random.Random(0xC0 + kidx).randrange(1, N)
        cases = [("n", which, sign) for which in range(3) for sign in (1, -1)] + [("final-dbl", 0, 1), ("acc3-inf", 0, -1),
                                                                                   ("total-inf", 0, -1)]
        for kind, which, sign in cases:
            while True:
                u2 = rng.randrange(1, N)
                k1, k2 = ev.glv_halves(u2)
                w3 = [s for s in cold_chains(0, u2, c)["wave3"] if s[0] != "G"]
                if len(w3) < 3 or not k1:
                    continue
                if kind == "n":
                    at = _targets(w3)[which]
                    u1 = (sign * w3[at][1] - sum(x for _, x in w3[:at])) % N
                    target = ("wave3", w3[at][0])
                elif kind == "final-dbl":
                    u1, target = c * (k1 - ev.LAMBDA * k2) % N, ("wave1", "acc3")
                elif kind == "acc3-inf":
                    u1, target = -c * ev.LAMBDA * k2 % N, ("wave3", w3[-1][0])
                else:
                    u1, target = -c * u2 % N, ("wave1", "acc3")
                rs = sign_for(c, u1, u2) if u1 else None
                if rs:
                    break
            tag = f"cold/k{kidx}/{kind}{which}/{'dbl' if sign > 0 else 'inv'}"
            out.append(Vec(tag, c, u1, u2, rs[0], rs[1], target, sign))
    _CACHE["cold"] = out
    return out


def _forms(u1, u2, geom):
    """The warm tree's leaves as linear forms (a, b) standing for a + b c."""
    w, nwin, _ = WARM_GEOMETRIES[geom]
    leaves = [((d << (GW * j)) % N, 0) for j, d in enumerate(ev.signed_digits(u1, GW, GNWIN))]
    for h, k in enumerate(ev.glv_halves(u2)):
        for j, d in enumerate(ev.signed_digits(abs(k), w, nwin)):
            leaves.append((0, (-d if k < 0 else d) * (1 << (w * j)) * (ev.LAMBDA if h else 1) % N))
    return leaves


def _fsum(fs):
    return (sum(a for a, _ in fs) % N, sum(b for _, b in fs) % N)


def warm_tree(u1, u2, geom):
    """{name: [(label, form)]} of every addition chain of the warm tree, in
    linear forms: the leaf pairs, each wave's range of nodes, the 4 -> 2
    level and the root."""
    split = small_constants()["kWarmSplit"][geom]
    leaves = _forms(u1, u2, geom)
    chains, nodes = {}, []
    for i in range((len(leaves) + 1) // 2):
        pair = leaves[2 * i:2 * i + 2]
        chains[f"pair{i}"] = [((2 * i + t), f) for t, f in enumerate(pair)]
        nodes.append(_fsum(pair))
    assert len(nodes) == split[4]
    cs = []
    for wv in range(4):
        rng_ = range(split[wv], split[wv + 1])
        chains[f"wave{wv}"] = [(i, nodes[i]) for i in rng_]
        cs.append(_fsum([nodes[i] for i in rng_]))
    a = []
    for wv in range(2):
        chains[f"level2/{wv}"] = [(2 * wv + t, cs[2 * wv + t]) for t in range(2)]
        a.append(_fsum(cs[2 * wv:2 * wv + 2]))
    chains["root"] = [(0, a[0]), (1, a[1])]
    return chains


def warm_chains(u1, u2, c, geom):
    """warm_tree evaluated at c: {name: steps} in scalars."""
    return {name: [(label, (a + b * c) % N) for label, (a, b) in steps] for name, steps in warm_tree(u1, u2, geom).items()}


def warm_targets(geom):
    """(chain, label) of the cross-chain additions: in wave ranges, a key
    node added to a sum that still holds generator leaves only or both kinds;
    the 4 -> 2 addition of waves 0 and 1's sums; the root."""
    split = small_constants()["kWarmSplit"][geom]
    out = []
    for wv in range(4):
        nodes = list(range(split[wv], split[wv + 1]))
        if nodes[0] < GNWIN // 2:  # the range starts with generator pairs
            out += [(f"wave{wv}", i) for i in nodes if i >= GNWIN // 2]
    return out + [("level2/0", 1), ("root", 1)]


def warm_vectors(geom):
    """k_small's warm tree for one cached geometry: every cross-chain
    addition (warm_targets) as a doubling and as P + (-P), each on a key of
    its own (solved for c), and two plain vectors whose generator and key
    leaf pairs are partly both zero digits (u1 < 2^40, u2 < 2^20: identity
    nodes handed over), on the first of those keys."""
    key = ("warm", geom)
    if key in _CACHE:
        return _CACHE[key]
    rng = random.Random(0x3A23 + WARM_GEOMETRIES[geom][0])
    out = []
    for chain, label in warm_targets(geom):
        for sign in (1, -1):
            while True:
                u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
                steps = warm_tree(u1, u2, geom)[chain]
                at = [i for i, (lb, _) in enumerate(steps) if lb == label][0]
                (a1, b1), (a2, b2) = _fsum([f for _, f in steps[:at]]), steps[at][1]
                num, den = (sign * a2 - a1) % N, (b1 - sign * b2) % N
                if not num or not den:
                    continue
                c = num * pow(den, -1, N) % N
                rs = sign_for(c, u1, u2)
                if rs:
                    break
            tag = f"warm{geom}/{chain}/{label}/{'dbl' if sign > 0 else 'inv'}"
            out.append(Vec(tag, c, u1, u2, rs[0], rs[1], (chain, label), sign))
    c0 = out[0].c
    for i in range(2):
        while True:
            u1, u2 = rng.randrange(1, 1 << 40), rng.randrange(1, 1 << 20)
            rs = sign_for(c0, u1, u2)
            if rs:
                break
        out.append(Vec(f"warm{geom}/identity-nodes/{i}", c0, u1, u2, rs[0], rs[1], None, 0))
    _CACHE[key] = out
    return out
