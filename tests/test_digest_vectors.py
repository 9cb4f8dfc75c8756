"""The digest edge vectors of tests/digest_vectors.py on the CPU: e = 0 and
e = N (u1 = 0: the generator chain leaves the identity), e >= N up to
2^256 - 1 (the digest is read unreduced), limb patterns of e, a generator half
that is empty over a wave's range, and the twins that must REJECT.

What is held here: the vector and REJECT counts; each family's construction
invariants in Python integers; three judges over the supplied digests
(oracle.gosemantics.item_status, the C oracle, OpenSSL where it is there)
against the status the construction fixes; that no order model of
tests/test_chain_exceptions.py reports an exceptional addition for any vector
(an identity accumulator taking an entry is none); and the kernels' own source
on the host, tests/deferexc in its digests-in mode in both builds of
tests/test_chain_exceptions.py, for K12, K8, KC22 and KC18: the device order
and the host entries' order decide what the construction says, and no call
takes the second pass.  The generic path and k_small have no host build:
their only execution of these vectors is tests/test_gpu_digest_vectors.py."""
import pytest

from oracle import coracle
from oracle import gosemantics as gs
from oracle import openssl_xcheck
from tests import chain_vectors as cv
from tests import digest_vectors as dg
from tests import edge_vectors as ev
from tests import test_chain_exceptions as tce
from tests.test_chain_exceptions import host_replay_exe, replay_exe  # noqa: F401  (fixtures: the two builds)

N = dg.N


def test_counts_and_tags():
    vecs = dg.vectors()
    assert len(vecs) == dg.N_VECTORS == sum(n for n, _ in dg.COUNTS.values())
    assert sum(v.want == gs.REJECT for v in vecs) == dg.N_REJECT == sum(r for _, r in dg.COUNTS.values())
    assert len({v.tag for v in vecs}) == len(vecs)
    for f, (n, n_reject) in dg.COUNTS.items():
        fam = dg.family(f)
        assert len(fam) == n and sum(v.want == gs.REJECT for v in fam) == n_reject, f
        assert all(v.want in (gs.ACCEPT, gs.REJECT) for v in fam)
    # both of cv.k_vectors("K12")'s keys in every family but t/ (one key is enough there)
    for f in "zngx":
        assert {v.c for v in dg.family(f)} == set(dg.keys()), f
    assert {v.pub for v in vecs} == {v.pub for v in cv.k_vectors("K12")}


def test_recovered_scalars_are_the_kernels():
    """u1, u2 and total of every vector are what verification forms from
    (digest, r, s): e unreduced times s^-1 mod N."""
    for v in dg.vectors():
        w = pow(v.s, -1, N)
        assert 0 < v.r < N and 0 < v.s < N, v.tag
        assert (v.u1, v.u2) == (v.e * w % N, v.r * w % N) and v.u2, v.tag
        assert v.total == (v.u1 + v.u2 * v.c) % N and v.total, v.tag
        x = gs.scalar_mult(v.total, gs.G)[0]
        assert (x % N == v.r) == (v.want == gs.ACCEPT), v.tag


def test_family_z_has_no_generator_part():
    zs = dg.family("z")
    assert {v.tag.split("/")[1] for v in zs} == {"rand", "N", "one", "minus-one", "lambda", "half0", "half1"}
    for v in zs:
        assert v.e % N == 0 and v.e in (0, N) and v.u1 == 0 and v.want == gs.ACCEPT, v.tag
        # every generator pair of the warm tree is the identity, on both cached geometries
        for geom in cv.WARM_GEOMETRIES:
            chains = cv.warm_chains(v.u1, v.u2, v.c, geom)
            for i in range(cv.GNWIN // 2):
                assert all(x == 0 for _, x in chains[f"pair{i}"]), (v.tag, geom, i)
            n_pairs = cv.small_constants()["kWarmSplit"][geom][4]
            assert any(x for i in range(cv.GNWIN // 2, n_pairs) for _, x in chains[f"pair{i}"]), (v.tag, geom)
    assert {v.e for v in zs} == {0, N}
    by = {v.tag: v for v in zs}
    for k in ("k0", "k1"):
        assert (by[f"z/rand/{k}"].r, by[f"z/rand/{k}"].s) == (by[f"z/N/{k}"].r, by[f"z/N/{k}"].s)
        assert by[f"z/one/{k}"].u2 == 1 and by[f"z/one/{k}"].s == by[f"z/one/{k}"].r
        assert by[f"z/one/{k}"].r == gs.Unmarshal(by[f"z/one/{k}"].pub)[0] % N  # R = Q
        assert by[f"z/minus-one/{k}"].u2 == N - 1 and by[f"z/lambda/{k}"].u2 == ev.LAMBDA
        h0, h1 = ev.glv_halves(by[f"z/half0/{k}"].u2), ev.glv_halves(by[f"z/half1/{k}"].u2)
        assert h0[1] == 0 and h1[0] == 0 and h0[0] == h1[1] and h0[0].bit_length() == 127, (h0, h1)
        assert ev.glv_halves(N - 1) == (-1, 0) and ev.glv_halves(ev.LAMBDA) == (0, 1)
    # the low-s convention is not imposed: s = r where u2 = 1, s = -r where u2 = -1
    assert any(v.s > (N - 1) // 2 for v in zs)


def test_family_n_digests_are_at_or_above_n():
    ns = dg.family("n")
    by = {v.tag: v for v in ns}
    seen = set()
    for v in ns:
        if "/hi/" not in v.tag:
            continue
        lo = by[v.tag.replace("/hi/", "/lo/")]
        assert v.e >= N and v.e == lo.e + N and 0 < lo.e < dg.TOP - N, v.tag
        assert (v.r, v.s, v.c) == (lo.r, lo.s, lo.c) and v.u1 == lo.u1 and v.want == lo.want == gs.ACCEPT, v.tag
        seen.add(lo.e)
    assert {1, 1 << 32, 1 << 128, dg.TOP - N - 1} <= seen and len(seen) == 5


def test_family_t_values():
    ts = dg.family("t")
    assert [v.e for v in ts] == [e for _, e in dg.T_VALUES]
    assert {dg.TOP - 1, dg.TOP - (1 << 32), N - 1, N + 1, 1 << 255, 1, (1 << 224) - 1, (1 << 32) - 1} == {v.e for v in ts}
    assert all(v.want == gs.ACCEPT for v in ts)


def test_family_g_empties_wave_zero():
    """u1 < N is a multiple of 2^(26 * 6), of 2^(26 * 8), or the top window
    alone (the 6 and 8 from kWarmSplit): in cv.warm_chains every node of wave
    0's range is the identity on KC22 or KC18, while u1 != 0."""
    shifts = dict(dg.g_shifts())
    assert shifts == {"wave0-KC22": 26 * 6, "wave0-KC18": 26 * 8, "top-window": 26 * 9}
    for v in dg.family("g"):
        bits = shifts[v.tag.split("/")[1]]
        assert 0 < v.u1 < N and v.u1 % (1 << bits) == 0 and v.e == v.u1 * v.s % N and v.want == gs.ACCEPT, v.tag
        digits = ev.signed_digits(v.u1, cv.GW, cv.GNWIN)
        assert not any(digits[:bits // cv.GW]) and any(digits), v.tag
        if "top-window" in v.tag:
            assert sum(1 for d in digits if d) == 1 and digits[-1] > 0, v.tag
        empty = []
        for geom in cv.WARM_GEOMETRIES:
            chains = cv.warm_chains(v.u1, v.u2, v.c, geom)
            if all(x == 0 for _, x in chains["wave0"]):
                empty.append(geom)
        assert empty, v.tag
        if "KC18" in v.tag or "top" in v.tag:
            assert empty == ["KC22", "KC18"], v.tag


def test_family_x_twins_reject():
    xs = dg.family("x")
    by = {v.tag: v for v in dg.vectors()}
    assert all(v.want == gs.REJECT for v in xs) and len(xs) >= 10
    n = 0
    for k in ("k0", "k1"):
        for name, src in (("z-rand", f"z/rand/{k}"), ("z-one", f"z/one/{k}")):
            for e_name, e in (("e=1", 1), ("e=N+1", N + 1)):
                t = by[f"x/{name}/{e_name}/{k}"]
                assert (t.r, t.s, t.c, t.e, t.u1 != 0) == (by[src].r, by[src].s, by[src].c, e, True), t.tag
                n += 1
        for e_name, e in (("e=0", 0), ("e=N", N)):
            t = by[f"x/valid-under-1/{e_name}/{k}"]
            assert t.e == e and t.u1 == 0, t.tag
            assert gs.item_status(t.pub, (1).to_bytes(32, "big"), t.r, t.s) == gs.ACCEPT, t.tag
            n += 1
        for name in dg.E0_NAMES:
            t, src = by[f"x/n-{name}-hi/e-1/{k}"], by[f"n/{name}/hi/{k}"]
            assert (t.r, t.s, t.c, t.e) == (src.r, src.s, src.c, src.e - 1) and t.e >= N, t.tag
            n += 1
    t, src = by["x/t-2^256-1/e-1"], by["t/2^256-1"]
    assert (t.r, t.s, t.c, t.e) == (src.r, src.s, src.c, dg.TOP - 2)
    assert n + 1 == len(xs)
    # the twins whose accumulator is the identity after the generator chain
    assert sum(v.u1 == 0 for v in xs) == 6


def test_three_judges_agree_with_the_construction():
    ossl = openssl_xcheck.available()
    for v in dg.vectors():
        assert gs.item_status(v.pub, v.digest, v.r, v.s) == v.want, v.tag
        assert coracle.item_status(v.pub, v.digest, 0, v.r.to_bytes(32, "big"), v.s.to_bytes(32, "big")) == v.want, v.tag
        if ossl:
            assert openssl_xcheck.verify(v.pub, v.digest, v.r, v.s) == (v.want == gs.ACCEPT), v.tag


def test_no_order_model_reports_an_exceptional_addition():
    """Every vector in every family model of tests/test_chain_exceptions.py:
    u1 = 0 is a zero step (nothing added) and an identity accumulator taking
    an entry is no collision."""
    for v in dg.vectors():
        for fam in tce.FAMILIES:
            assert cv.all_collisions(tce.model(fam, v)) == [], (v.tag, fam)


def _fillers():
    return [p for i, c in enumerate(dg.keys()) for p in cv.plain(0xD1F1 + i, 2, c)]


@pytest.mark.parametrize("geom", ["K12", "K8", "KC22", "KC18"])
def test_host_replay_device_order(replay_exe, tmp_path, geom):  # noqa: F811
    """verify_item_g + verify_item_q<K12 | K8> and verify_item_gq_kc<22 | 18>
    compiled for the host (the emulator's generator windows), and the host
    entries' order over the same tables: the construction's status from
    both, and no second pass anywhere."""
    vecs = dg.vectors() + _fillers()
    want, rows = tce.replay(replay_exe, vecs, geom, tmp_path)
    _check(vecs, want, rows)


@pytest.mark.parametrize("geom", ["K12", "K8", "KC22", "KC18"])
def test_host_replay_host_order(host_replay_exe, tmp_path, geom):  # noqa: F811
    """The build with the product's 26-bit generator windows over a sparse
    generator table (an item with u1 = 0 lists no slot and reads slot 0 of
    every window, which is not added): verify_item_qfirst<geom> then
    verify_item_gfinish, whose FINAL top window has d == 0 for u1 = 0, and
    the device order of the same build."""
    vecs = dg.vectors() + _fillers()
    want, rows = tce.replay(host_replay_exe, vecs, geom, tmp_path, sparse_g=True)
    _check(vecs, want, rows)


def _check(vecs, want, rows):
    bad = []
    for v, w, t in zip(vecs, want, rows):
        st_dev, st_host, redo_g, redo_q, redo_qf, redo_gf = (int(x) for x in t[2:8])
        assert w == v.want
        if not (st_dev == st_host == w and redo_g == redo_q == redo_qf == redo_gf == 0):
            bad.append(f"{v.tag}: want {w} dev {st_dev} host {st_host} redo g{redo_g} q{redo_q} qf{redo_qf} gf{redo_gf}")
    assert not bad, f"{len(bad)} of {len(vecs)}: " + "; ".join(bad)
