"""The chosen-scalar edge vectors (tests/edge_vectors.py) on the CPU: their
statuses by Python integers, by the C oracle and by the host build of the
device code in every forced mode, and — by assertion on each vector's real
u1 and GLV halves — that the set offers every (window, digit class) pair of
every table geometry, every k_small cold-scheduler pattern and both sides of
the final check's `r < p - N` guard.  tests/test_gpu_edge_vectors.py runs the
same vectors through the real kernels; for the paths only the GPU has (the
26-bit generator windows, the KC tables, k_small's phases) the coverage
assertions here are the evidence that the patterns are offered.
"""
import hashlib
import subprocess

import numpy as np
import pytest

from oracle import coracle
from tests import edge_vectors as ev
from tests.emu import emu
from tests.helpers import bits_from_status

P, N = ev.P, ev.N

# (window, class) pairs no scalar offers, by name.  All are top-window cases:
# the top window of a geometry holds only the bits its scalar has left
# (u1 < N < 2^256; a GLV half stays below about 2^127.6), and a class whose
# smallest value (edge_vectors.class_value) needs more bits cannot occur.
# test_dropped_pairs_are_out_of_reach checks each entry against that rule.
_UPPER = ("half-1", "half", "half+1", "full", "full+carry")
DROPPED = {
    "G26x10": {9: _UPPER},                       # 22 bits left of a 26-bit window
    "G22x12": {11: _UPPER},                      # 14 of 22
    "G16x17": {16: ("sub-1", "sub", "sub+1", "m*sub", "below-sub") + _UPPER},  # the last carry alone: 0 or 1
    "K12": {10: _UPPER},                         # 8 of 12
    "K8": {15: ("full",)},                       # 255 2^120 is above every half the split returns
    "KC": {5: _UPPER},                           # 18 of 22
}


@pytest.fixture(scope="module")
def vs():
    return ev.vectors()


@pytest.fixture(scope="module")
def halves(vs):
    """Each vector's GLV halves from the product's own split, so the
    coverage statements below describe what the device will see."""
    return [emu_glv_halves(v.u2) for v in vs]


def emu_glv_halves(u2):
    """(k1, k2), signed, of the product's own split (the CPU build of
    field.h's glv_split), as test_emu.py calls it."""
    import ctypes

    L = emu.lib()
    L.emu_glv_split.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    kin = np.array([(u2 >> (32 * i)) & 0xFFFFFFFF for i in range(8)], np.uint32)
    out = np.zeros(9, np.uint32)
    L.emu_glv_split(kin.ctypes.data, out.ctypes.data)
    m1 = sum(int(out[i]) << (32 * i) for i in range(4))
    m2 = sum(int(out[4 + i]) << (32 * i) for i in range(4))
    return (-m1 if out[8] & 1 else m1), (-m2 if out[8] & 2 else m2)


def _tags(vs, idx):
    return [vs[i].tag for i in idx]


def test_generation_is_deterministic_and_sized(vs):
    assert 300 <= len(vs) <= 400
    assert {v.family for v in vs} == set("abcde")
    again = ev.generate()
    assert [(v.tag, v.body, v.pub, v.r, v.s) for v in again.out] == [(v.tag, v.body, v.pub, v.r, v.s) for v in vs]
    assert again.dropped == ev.dropped()


def test_split_model_is_the_products_split(vs, halves):
    """The generator filters half patterns with a Python-integer model of
    glv_split (so that it also runs where the emulator is not built): equal
    to the product's split on every vector, on every pattern it dropped (the
    product's split does not return those either) and on random scalars."""
    assert [ev.glv_halves(v.u2) for v in vs] == halves
    for tag, k1, k2 in ev.dropped():
        u2 = (k1 + k2 * ev.LAMBDA) % N
        assert emu_glv_halves(u2) == ev.glv_halves(u2) != (k1, k2), tag
    rng = np.random.default_rng(6)
    ks = [0, 1, N - 1, (N - 1) // 2, (N + 1) // 2, ev.LAMBDA]
    for k in ks + [int.from_bytes(rng.bytes(32), "big") % N for _ in range(2000)]:
        k1, k2 = ev.glv_halves(k)
        assert (k1, k2) == emu_glv_halves(k) and (k1 + k2 * ev.LAMBDA - k) % N == 0


def test_models():
    rng = np.random.default_rng(5)
    for g in ev.G_GEOMETRIES + (ev.K12, ev.KC):
        for _ in range(200):
            u = int.from_bytes(rng.bytes(g.bits // 8), "big") % (N if g.bits == 256 else 1 << 127)
            d = ev.signed_digits(u, g.W, g.NWIN)
            half = 1 << (g.W - 1)
            assert sum(x << (g.W * j) for j, x in enumerate(d)) == u and all(-half < x <= half for x in d)
    ks = [0, 1, 2, 3, 7, (1 << 127) - 1, int("01" * 63, 2)]
    for k in ks + [int.from_bytes(rng.bytes(16), "big") for _ in range(200)]:
        d = ev.naf(k)
        assert sum(x << i for i, x in enumerate(d)) == k
        assert all(not (a and b) for a, b in zip(d, d[1:]))


def test_statuses_python_construction_oracle(vs):
    """Direct verification in Python integers gives the status each vector's
    construction fixes, and the C oracle gives the same."""
    st = ev.direct_statuses()
    bad = [i for i, v in enumerate(vs) if st[i] != v.expect]
    assert not bad, _tags(vs, bad)
    h, ost, bits = coracle.verify_batch(ev.batch().as_dict())
    bad = np.flatnonzero(ost != st)
    assert bad.size == 0, _tags(vs, bad)
    assert [h[i].tobytes() for i in range(len(vs))] == [hashlib.sha256(v.body).digest() for v in vs]
    assert np.array_equal(bits, bits_from_status(st))
    assert 0 < int((st == 0).sum()) < len(vs)


# 5 / 6: K8 / K12 with the key part first, reported as modes 1 / 2 (as test_emu.py)
@pytest.mark.parametrize("mode", [2, 1, 0, 3, 5, 6])
def test_emulator_modes(vs, mode):
    st = ev.direct_statuses()
    b = ev.batch()
    h, est, bits, m = emu.verify_batch(b.as_dict(), force_mode=mode)
    assert m == (mode - 4 if mode >= 5 else mode)
    bad = np.flatnonzero(est != st)
    assert bad.size == 0, f"emulator mode {mode}: {_tags(vs, bad)} got {est[bad]} want {st[bad]}"
    assert np.array_equal(bits, bits_from_status(st))
    assert h[0].tobytes() == hashlib.sha256(vs[0].body).digest()


def _scalars(g, vs, halves, idx=None):
    """The scalars geometry g recodes: u1, or each half's magnitude with the
    half it came from."""
    idx = range(len(vs)) if idx is None else idx
    if g.bits == 256:
        return [(0, vs[i].u1) for i in idx]
    return [(h, abs(halves[i][h])) for i in idx for h in (0, 1)]


def _required(g, j, top_bits=None):
    """Every class, in every window; `top_bits`: only what a top window of
    that many bits can hold."""
    classes = ev.SIGNED_CLASSES if g.signed else ev.UNSIGNED_CLASSES
    need = set(classes)
    if j == 0:
        need.discard("full+carry")  # no carry enters window 0
    if j == g.NWIN - 1 and top_bits is not None:
        need = {c for c in need if ev.class_value(g, c) < (1 << top_bits)}
    return need


def _missing(g, scalars, top_bits=None):
    seen = {}
    for h, u in scalars:
        for j, cs in enumerate(ev.window_classes(g, u)):
            seen.setdefault((h, j), set()).update(cs)
    out = []
    for h in sorted({h for h, _ in scalars}):
        for j in range(g.NWIN):
            for c in sorted(_required(g, j, top_bits) - seen.get((h, j), set())):
                out.append((g.name, f"k{h + 1}" if g.bits == 128 else "u1", j, c))
    return out


@pytest.mark.parametrize("g", ev.G_GEOMETRIES + ev.K_GEOMETRIES, ids=lambda g: g.name)
def test_every_window_meets_every_class(vs, halves, g):
    """Windows: for every window of the geometry (for the key geometries: of
    each GLV half), every digit class occurs in some vector, except the
    top-window pairs DROPPED names."""
    missing = _missing(g, _scalars(g, vs, halves))
    named = {(j, c) for j, cs in DROPPED[g.name].items() for c in cs}
    assert not [m for m in missing if (m[2], m[3]) not in named], "not offered and not on DROPPED"
    assert named == {(m[2], m[3]) for m in missing}, "on DROPPED but offered: take it off"


def test_dropped_pairs_are_out_of_reach(vs, halves):
    """DROPPED is short, names top windows only, and every pair on it needs a
    window value the scalar cannot have: above the bits left for u1 < 2^256,
    or at a half of at least 2^127.6 (the split's halves end at the corners
    (+-v1 +-v2) / 2 of its lattice cell: |k1| < 2^127.35, |k2| < 2^127.12)."""
    assert sum(len(cs) for w in DROPPED.values() for cs in w.values()) <= 36
    for g in ev.G_GEOMETRIES + ev.K_GEOMETRIES:
        for j, cs in DROPPED[g.name].items():
            assert j == g.NWIN - 1
            for c in cs:
                v = ev.class_value(g, c) << (g.W * j)
                assert v >= (1 << 256 if g.bits == 256 else int(2 ** 127.6)), (g.name, c)
    # what the generator itself gave up: only halves that are not both below 2^126
    for tag, k1, k2 in ev.dropped():
        assert max(abs(k1), abs(k2)) >= 1 << ev.SAFE_HALF_BITS, tag
    assert sorted(t for t, _, _ in ev.dropped()) == sorted([
        "b/K8/top-full/k1", "b/K8/top-full/k2", "b/max/k1=0,k2=0x7fffffffffffffffffffffffffffffff",
        "b/max/k1=0,k2=0x80000000000000000000000000000000", "c/empty/2^127/+-"])
    tags = {v.tag for v in vs}
    assert {"b/max/k1=0x7fffffffffffffffffffffffffffffff,k2=0",
            "b/max/k1=0x80000000000000000000000000000000,k2=0"} <= tags
    # the largest magnitudes: both halves reach past 2^127
    assert max(abs(k1) for k1, _ in halves) > 1 << 127 and max(abs(k2) for _, k2 in halves) > 1 << 127


def test_half_patterns_round_trip_with_every_sign_pair(vs, halves):
    """Family b and c vectors carry exactly the halves and signs they were
    built from; every rotation of K12 and K8 occurs with all four sign pairs,
    KC's rotations share the four among them; k1 = 0, k2 = 0, k1 = +-k2."""
    for v, k in zip(vs, halves):
        if "k" in v.meta:
            assert v.meta["k"] == k, v.tag
    for g, ncls in ((ev.K12, 12), (ev.K8, 7), (ev.KC, 12)):
        tags = {v.tag for v in vs}
        for rot in range(ncls):
            pairs = {sp for sp in ("++", "-+", "+-", "--") if f"b/{g.name}/rot{rot}/{sp}" in tags}
            assert len(pairs) == (1 if g is ev.KC else 4), (g.name, rot)
        assert {sp for sp in ("++", "-+", "+-", "--") for rot in range(ncls)
                if f"b/{g.name}/rot{rot}/{sp}" in tags} == {"++", "-+", "+-", "--"}
        by_tag = {v.tag: k for v, k in zip(vs, halves)}
        assert by_tag[f"b/{g.name}/k1=0"][0] == 0 and by_tag[f"b/{g.name}/k1=0"][1] != 0
        assert by_tag[f"b/{g.name}/k2=0"][1] == 0 and by_tag[f"b/{g.name}/k2=0"][0] != 0
        k1, k2 = by_tag[f"b/{g.name}/k1=k2"]
        assert k1 == k2 != 0
        k1, k2 = by_tag[f"b/{g.name}/k1=-k2"]
        assert k1 == -k2 != 0


def test_from_identity_shapes_and_carry_chains(vs, halves):
    """The three start-from-identity shapes (window 0 zero and window 1 not,
    the reverse, both zero) in u1 for every generator geometry and in each
    half for every key geometry; a carry through every window boundary; u1
    with exactly one non-zero window, for each window; u1 in {1, 2, N-1,
    N-2}; the carry out of bit 255 in the 16-bit geometry's last window."""
    def shapes(g, scalars):
        out = set()
        for u in scalars:
            d = ev.signed_digits(u, g.W, g.NWIN) if g.signed else ev.unsigned_digits(u, g.W, g.NWIN)
            if u and any(d[2:]):
                out.add((d[0] != 0, d[1] != 0))
        return out

    for g in ev.G_GEOMETRIES:
        u1s = [v.u1 for v in vs]
        assert shapes(g, u1s) >= {(False, True), (True, False), (False, False)}, g.name
        digits = [ev.signed_digits(u, g.W, g.NWIN) for u in u1s]
        for j in range(1, g.NWIN):
            if g.W * j < 256:  # 2^(W j) - 1: -1, then a carry through j - 1 windows, landing as +1 in window j
                want = [-1] + [0] * (j - 1) + [1] + [0] * (g.NWIN - j - 1)
                assert want in digits and (1 << (g.W * j)) in u1s, (g.name, j)
        for j in range(g.NWIN):
            if g.W * j + 2 < 256:
                assert any(d[j] not in (0, 1) and not any(d[:j] + d[j + 1:]) for d in digits), (g.name, j)
    assert {1, 2, N - 1, N - 2} <= {v.u1 for v in vs}
    assert ev.signed_digits(N - 1, 16, 17)[16] == 1
    for g in ev.K_GEOMETRIES:
        for h in (0, 1):
            assert shapes(g, [abs(k[h]) for k in halves]) >= {(False, True), (True, False), (False, False)}, (g.name, h)


def test_naf_patterns_for_the_cold_scheduler(vs, halves):
    """NAF: every family c property holds on the halves the split really
    returns, for k1 (k_small's wave 1) and k2 (wave 3, which also adds the G
    sum in its first phase): the densest NAF, a burst of digits inside the 37
    pre-published entries, one digit alone at bits 0 / 36 / 37 / 126 and the
    top bit the split allows, 2^k - 1 runs, an empty half beside a dense one
    in both orders."""
    c = [(v.tag, [ev.naf(abs(k[0])), ev.naf(abs(k[1]))], k) for v, k in zip(vs, halves) if v.family == "c"]

    def nz(d):
        return [i for i, x in enumerate(d) if x]

    for h in (0, 1):
        o = 1 - h
        # the densest NAF: a digit at every second bit
        assert any(len(nz(d[h])) >= 63 and nz(d[h]) == list(range(nz(d[h])[0], nz(d[h])[-1] + 1, 2))
                   for _, d, _ in c), h
        burst = [t for t, d, _ in c if len(nz(d[h])) >= 12 and max(nz(d[h])) < 37]
        assert burst, h
        assert any(len(nz(d[h])) >= 12 and max(nz(d[h])) < 37 and len(nz(d[o])) >= 63 for _, d, _ in c), h
        for bit in (0, 36, 37, 126):
            assert any(nz(d[h]) == [bit] and not nz(d[o]) for _, d, _ in c), (h, bit)
        for k in (37, 38, 100, 126):
            assert any(d[h] == [-1] + [0] * (k - 1) + [1] for _, d, _ in c), (h, k)
        assert any(not nz(d[h]) and len(nz(d[o])) >= 63 for _, d, _ in c), h  # empty beside dense
        assert any(nz(d[h]) == [126] and len(nz(d[o])) >= 63 for _, d, _ in c), h
        assert any(k[h] < 0 for _, _, k in c) and any(k[h] > 0 for _, _, k in c)
    # the top bit: k1 alone reaches 2^127 (and 2^127 - 1, whose NAF ends at bit 127);
    # k2 alone does not (edge_vectors.dropped()), its highest single digit is bit 126
    assert any(nz(d[0]) == [127] and not nz(d[1]) for _, d, _ in c)
    assert any(d[0] == [-1] + [0] * 126 + [1] for _, d, _ in c)


def test_final_check_vectors(vs):
    """Wrap: every family d wrap vector has N <= x(R) < p and r = x(R) - N
    below p - N, and is accepted.  Guard: every guard vector has r >= p - N
    and x(R) = r + N - p (what a 256-bit r + N is as a field element below
    2^256) or r + N - 2^256 (what it wraps to above), and is rejected.  The
    r at / above p - N vectors have x(R) = r.  Every accepted wrap vector
    occurs with r and with s flipped in one bit, rejected."""
    st = ev.direct_statuses()
    kinds = {}
    for i, v in enumerate(vs):
        if v.family != "d":
            continue
        kind = v.meta["kind"]
        kinds.setdefault(kind, []).append(v)
        if kind == "flip":
            assert st[i] == 0, v.tag
            continue
        R = ev.total_point(v)
        assert R is not None and R[0] == v.meta["x"], v.tag
        if kind == "wrap":
            assert N <= R[0] < P and v.r == R[0] - N and v.r < P - N and st[i] == 1, v.tag
        elif kind == "plain":
            assert R[0] == v.r and st[i] == 1, v.tag
        elif kind == "guard":
            assert P - N <= v.r < N and R[0] == v.r + N - P and st[i] == 0, v.tag
        else:
            assert kind == "guard256" and (1 << 256) - N <= v.r < N and R[0] == v.r + N - (1 << 256) and st[i] == 0
    assert len(kinds["wrap"]) >= 4 and len(kinds["guard"]) >= 3 and len(kinds["guard256"]) >= 2
    xs = [v.meta["x"] for v in kinds["wrap"]]
    assert all(ev.lift_x(x) is None for x in range(max(xs) + 1, P))       # the largest liftable x below p
    assert all(ev.lift_x(x) is None for x in range(N + 1, min(xs)))       # and the smallest above N
    assert any(v.r + N < (1 << 256) for v in kinds["guard"])              # r + N - p without a 2^256 wrap
    plain = sorted(v.r for v in kinds["plain"])
    assert plain[0] < P - N <= plain[1] and all(ev.lift_x(x) is None for x in range(P - N, plain[1]))
    assert any(v.r == plain[0] for v in kinds["wrap"])                    # the last r the guard lets through
    for w in kinds["wrap"]:
        flips = [v for v in kinds["flip"] if v.tag.startswith(w.tag + "/flip-")]
        assert {(v.r != w.r, v.s != w.s) for v in flips} == {(True, False), (False, True)}, w.tag


def test_exceptional_totals(vs):
    """Family e: u1 G = u2 Q under a valid signature (the total is a
    doubling, ACCEPT) and u1 G = -u2 Q (the identity, REJECT) with recovered
    keys, and both totals with Q = G and Q = -G."""
    from oracle import gosemantics as gs

    st = ev.direct_statuses()
    seen = set()
    for i, v in enumerate(vs):
        if v.family != "e":
            continue
        q = gs.Unmarshal(v.pub)
        a, b = gs.scalar_mult(v.u1, gs.G), gs.scalar_mult(v.u2, q)
        small = q in (gs.G, (gs.G[0], P - gs.G[1]))
        if v.meta["kind"] == "double":
            assert a == b and st[i] == (0 if small else 1), v.tag
        else:
            assert a == (b[0], P - b[1]) and ev.total_point(v) is None and st[i] == 0, v.tag
        seen.add((v.meta["kind"], "G" if q == gs.G else "-G" if small else "recovered"))
    assert seen == {(k, q) for k in ("double", "infinity") for q in ("G", "-G", "recovered")}


def test_kc_subset_covers_the_kc_windows(vs, halves):
    """The vectors the GPU tests send through the key-cache tables (at most
    32 keys of 805 MB): families d and e whole, and for both halves every
    (window, class) pair of the KC geometry that the whole set offers."""
    idx = ev.kc_subset()
    b = ev.batch(idx)
    assert b.n_keys <= 32 and b.n_items == len(idx)
    assert {i for i, v in enumerate(vs) if v.family in "de"} <= set(idx)
    missing = _missing(ev.KC, _scalars(ev.KC, vs, halves, idx))
    assert {(m[2], m[3]) for m in missing} == {(5, c) for c in DROPPED["KC"][5]}, missing
    assert {(k[0] == 0, k[1] == 0) for k in (halves[i] for i in idx)} >= {(True, False), (False, True)}


def test_asan_ubsan_emulator_on_edge_vectors(vs, tmp_path):
    """The sanitized host build of the device code (tests/emu `make asan`:
    16-bit generator windows) on the vectors in its four modes, against the C
    oracle, as test_emu.py::test_asan_ubsan_emulator runs it: a stand-alone
    executable in a subprocess."""
    subprocess.run(["make", "-s", "-C", emu._HERE, "asan"], check=True)
    exe = emu._HERE + "/_build/emu_asan"
    path = str(tmp_path / "edge.bin")
    emu.dump_batch(path, ev.batch().as_dict())
    r = subprocess.run([exe, path, "4"], capture_output=True, text=True, timeout=600,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("equal") == 4 and "MISMATCH" not in r.stdout, r.stdout
    accepted = int((ev.direct_statuses() == 1).sum())
    assert r.stdout.count(f"{len(vs)} items, {accepted} accepted") == 4, r.stdout
