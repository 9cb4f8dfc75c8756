"""The field-boundary keys of tests/key_vectors.py on the CPU: what the vectors
cover, four judges of elliptic.Unmarshal on every key (Python integers,
oracle.gosemantics, the C oracle, OpenSSL's o2i_ECPublicKey), the forged
triples in Python integers and through the C oracle, the real-digest layouts
through the emulator (tests/emu: key_decode_one over the host build of
key_decode_point) in every key-table mode, and the forged triples through the
host replay of the per-lane chains with supplied digests (tests/deferexc).

What would go unseen without these keys: `!fe_ge_p(x) && !fe_ge_p(y)` in
key_decode_point deleted, or fe_ge_p wrong in any limb.  A twin (x' + p, y)
then decodes as (x', y): KS_OK where the reference panics."""
import numpy as np
import pytest

from oracle import coracle, openssl_xcheck
from oracle import gosemantics as gs
from tests import key_vectors as kv

P, N = kv.P, kv.N
EMU_MODES = [2, 1, 0, 3, 5, 6]  # tests/test_emu.py's: K12, K8, generic, mode 3, K8 / K12 with the key part first


def test_every_class_is_present():
    ks = kv.keys()
    tags = kv.by_tag()
    xs = kv.small_x_values()
    assert xs[:3] == [1, 2, 3] and 3 < xs[3] < 977 and not any(kv.ys_of(x) for x in range(xs[3] + 1, 977))
    assert xs[4] >= 977 and not any(kv.ys_of(x) for x in range(977, xs[4]))
    assert 2**32 - 2 <= xs[5] < 2**32
    assert xs[6] >= 2**32 and not any(kv.ys_of(x) for x in range(2**32, xs[6]))
    assert xs[7] <= kv.MAX_TWIN and not any(kv.ys_of(x) for x in range(xs[7] + 1, kv.MAX_TWIN + 1))
    assert not kv.ys_of(0)  # 7 is a non-residue: no point with x = 0
    for x in xs:  # both roots, each with its twin
        for i in (0, 1):
            good, bad = tags[f"x/{x}/y{i}"], tags[f"x+p/{x}/y{i}"]
            assert good.ok and not bad.ok and bad.x == good.x + P < 2**256 and bad.y == good.y
            assert gs.is_on_curve(bad.x, bad.y)  # the curve equation alone takes the twin
        assert tags[f"x/{x}/y0"].y + tags[f"x/{x}/y1"].y == P
    ys, all_roots = kv.small_y_values()
    assert min(ys) < 977 and any(2**32 - 16 <= y < 2**32 for y in ys) and any(2**32 <= y < 2**32 + 16 for y in ys)
    assert any(kv.MAX_TWIN - 16 <= y <= kv.MAX_TWIN for y in ys) and all_roots
    for y in ys:
        roots = kv.xs_of(y)
        assert len(set(roots)) == 3 and all(pow(x, 3, P) == (y * y - 7) % P for x in roots)
        for j in range(3 if y in all_roots else 1):
            lo, hi, bad = tags[f"y/{y}/r{j}/lo"], tags[f"y/{y}/r{j}/hi"], tags[f"y+p/{y}/r{j}"]
            assert lo.ok and hi.ok and not bad.ok and (lo.x, lo.y) == (roots[j], y) and hi.y == P - y
            assert bad.y == y + P < 2**256 and bad.x == lo.x and gs.is_on_curve(bad.x, bad.y)
    plain = {k.tag: k for k in ks if k.klass == "plain"}
    assert set(plain) == {"plain/x=p", "plain/y=p", "plain/ones", "plain/zero"}
    assert not any(k.ok for k in plain.values())
    assert plain["plain/x=p"].x == P and plain["plain/y=p"].y == P and plain["plain/zero"].pub == b"\x04" + bytes(64)
    assert plain["plain/ones"].pub == b"\x04" + b"\xff" * 64
    assert all(len(k.pub) == 65 and k.pub[0] == 4 for k in ks)  # the length and prefix classes are synth.adversarial's
    assert sum(k.ok for k in ks) == len({k.pub for k in ks if k.ok}) == 46 and len(ks) == 76


def test_twins_land_in_every_low_limb_case_of_fe_ge_p():
    """fe_ge_p with limbs 2..7 all ones: limb 1 == P1 decided by limb 0 >= P0;
    limb 1 > P1 with limb 0 wrapped below P0; limb 1 > P1 with limb 0 at or
    above P0.  (Limb 1 cannot itself wrap: the sum would pass 2^256.)"""
    want = {1: "limb1=P1,limb0>=P0", 2: "limb1=P1,limb0>=P0", 3: "limb1=P1,limb0>=P0", 976: "limb1=P1,limb0>=P0",
            977: "limb1>P1,limb0<P0", 2**32 - 1: "limb1>P1,limb0<P0", 4294967303: "limb1>P1,limb0>=P0",
            kv.MAX_TWIN: "limb1>P1,limb0>=P0"}
    assert sorted(want) == kv.small_x_values()
    for good, bad in kv.twins():
        v, res = (bad.x, good.x) if bad.klass == "x-twin" else (bad.y, good.y)
        assert res < P <= v < 2**256 and v - P == res
        case = kv.ge_p_case(v)
        assert case is not None, bad.tag
        if bad.klass == "x-twin":
            assert case == want[good.x], bad.tag
    for klass in ("x-twin", "y-twin"):
        cases = {kv.ge_p_case(b.x if klass == "x-twin" else b.y) for _, b in kv.twins() if b.klass == klass}
        assert cases == {"limb1=P1,limb0>=P0", "limb1>P1,limb0<P0", "limb1>P1,limb0>=P0"}, (klass, cases)
    # the extremes: x' + p = p + 1 (limb 0 = P0 + 1) and 2^256 - 1 (every limb all ones)
    assert kv.by_tag()["x+p/1/y0"].x == P + 1 and kv.by_tag()[f"x+p/{kv.MAX_TWIN}/y0"].x == 2**256 - 1
    assert kv.limbs(P + 977)[:2] == [0, kv.P1 + 1]  # where limb 0 wraps to zero


def test_ge_p_case_model():
    assert kv.ge_p_case(P) == "limb1=P1,limb0>=P0" and kv.ge_p_case(P - 1) is None
    assert kv.ge_p_case(P - 2**32) is None and kv.ge_p_case(2**256 - 1) == "limb1>P1,limb0>=P0"
    assert kv.limbs(P)[:2] == [kv.P0, kv.P1] == [0xFFFFFC2F, 0xFFFFFFFE] and set(kv.limbs(P)[2:]) == {0xFFFFFFFF}


def test_top_of_range_keys_differ_from_p_in_the_named_limb():
    """Canonical keys (OK) that a wrong fe_ge_p would flag: limb 0 just below
    P0; limb 1 below P1 with limb 0 at most / above P0; for each limb
    i = 2..7 that limb 0xFFFFFFFE under limbs 0 and 1 above P0 and P1 (an
    `hi` AND that skips limb i takes them for >= p)."""
    top = [k for k in kv.keys() if k.klass.startswith("top")]
    assert all(k.ok and k.x < P for k in top)
    by = {}
    for k in top:
        by.setdefault(k.klass, []).append(k)
    assert [P - k.x for k in by["top-limb0"]] == [3, 4]  # the two smallest on-curve distances below p
    assert not kv.ys_of(P - 1) and not kv.ys_of(P - 2)
    for k in by["top-limb0"]:
        assert kv.first_limb_below_p(k.x) == 0 and kv.limbs(k.x)[0] == kv.P0 - (P - k.x)
    (k,) = by["top-limb1"]
    assert kv.first_limb_below_p(k.x) == 1 and kv.limbs(k.x)[1] == kv.P1 - 1 and kv.limbs(k.x)[0] >= 0xFFFFF000
    (k,) = by["top-hi1"]
    assert kv.first_limb_below_p(k.x) == 1 and kv.limbs(k.x)[1] == kv.P1 - 1 and kv.limbs(k.x)[0] > kv.P0
    for i in range(2, 8):
        (k,) = by[f"top-hi{i}"]
        v = kv.limbs(k.x)
        assert kv.first_limb_below_p(k.x) == i and v[i] == 0xFFFFFFFE and v[0] > kv.P0 and v[1] > kv.P1, k.tag
        assert all(v[j] == 0xFFFFFFFF for j in range(1, 8) if j != i), k.tag
    assert set(by) == {"top-limb0", "top-limb1"} | {f"top-hi{i}" for i in range(1, 8)}


def test_four_judges_agree_on_every_key():
    ossl = openssl_xcheck.available()
    rng_digest = bytes(range(32))
    for k in kv.keys():
        assert (gs.Unmarshal(k.pub) is not None) == k.ok, k.tag
        assert coracle.lib().oracle_unmarshal(k.pub, 65, None) == (1 if k.ok else 0), k.tag
        if ossl:
            accepted = openssl_xcheck.verify(k.pub, rng_digest, 1, 1) is not None
            assert accepted == k.ok, k.tag
    if not ossl:
        pytest.skip("libcrypto not present: three judges agreed, the OpenSSL judge did not run")


def test_forged_triples_verify_in_python_integers():
    """Each (e, r, s) is a valid signature under its OK key by the textbook
    equation in Python integers, with the conventions of the other vector
    sets; the twin's items carry the same triple."""
    items = kv.forged_items()
    by = {v.tag: v for v in items}
    assert len(by) == len(items)
    n_accept = 0
    for v in items:
        if v.want != gs.ACCEPT:
            continue
        n_accept += 1
        assert v.key.ok and v.r % N and 0 < v.s <= (N - 1) // 2, v.tag
        w = pow(v.s, -1, N)
        u1, u2 = int.from_bytes(v.digest, "big") * w % N, v.r * w % N
        R = gs.point_add(gs.scalar_mult(u1, gs.G), gs.scalar_mult(u2, (v.key.x, v.key.y)))
        assert R is not None and R[0] % N == v.r, v.tag
    assert n_accept == sum(k.ok for k in kv.keys())  # every OK key decodes to limbs that must feed the math
    for good, bad in kv.twins():
        a, p, rn, s0 = (by[f"forged/{good.tag}"], by[f"forged/{bad.tag}"], by[f"forged/{bad.tag}/r=N"],
                        by[f"forged/{bad.tag}/s=0"])
        assert (p.digest, p.r, p.s, p.want) == (a.digest, a.r, a.s, gs.REF_PANIC)
        assert (rn.digest, rn.r, rn.s, rn.want) == (a.digest, N, a.s, gs.REJECT)
        assert (s0.digest, s0.r, s0.s, s0.want) == (a.digest, a.r, 0, gs.REJECT)


def test_oracles_give_every_forged_item_its_status():
    for v in kv.forged_items():
        assert gs.item_status(v.pub, v.digest, v.r, v.s) == v.want, v.tag
        r_be, s_be = v.r.to_bytes(32, "big"), v.s.to_bytes(32, "big")
        assert coracle.item_status(v.pub, v.digest, 0, r_be, s_be) == v.want, v.tag
        if v.want == gs.ACCEPT and openssl_xcheck.available():
            assert openssl_xcheck.verify(v.pub, v.digest, v.r, v.s) is True, v.tag


def test_layouts_put_every_key_at_every_alignment_and_one_last():
    lay = kv.layouts()
    seen = {}
    for s in range(4):
        b, tags = lay[f"shift{s}"]
        assert b.n_keys == b.n_items == len(kv.keys()) + 1 and len(b.key(0)) == s
        for k in range(1, b.n_keys):
            assert b.key(k) == kv.by_tag()[tags[k]].pub
            seen.setdefault(tags[k], set()).add(int(b.key_off[k]) & 3)
    assert set(seen) == set(kv.by_tag()) and all(v == {0, 1, 2, 3} for v in seen.values())
    b, tags = lay["last"]
    assert tags[-1] == kv.LAST_KEY and int(b.key_off[-1]) == b.key_bytes.size
    assert b.key(b.n_keys - 1) == kv.by_tag()[kv.LAST_KEY].pub
    assert not kv.by_tag()[kv.LAST_KEY].ok


@pytest.fixture(scope="module")
def layout_statuses():
    """{layout: expected statuses}: gosemantics.item_status, equal to the C
    oracle's, REJECT under the OK keys and REF_PANIC under the others."""
    out = {}
    for name, (b, tags) in kv.layouts().items():
        want = kv.expected(b)
        h, st, bits = coracle.verify_batch(b.as_dict())
        assert np.array_equal(st, want), name
        ok = {k.tag: k.ok for k in kv.keys()}
        assert [int(x) for x in want] == [gs.REJECT if ok.get(t) else gs.REF_PANIC for t in tags], name
        out[name] = (h, want, bits)
    return out


@pytest.mark.parametrize("mode", EMU_MODES)
def test_emulator_statuses_in_every_key_table_mode(layout_statuses, mode):
    from tests.emu import emu

    for name, (b, tags) in kv.layouts().items():
        h, want, bits = layout_statuses[name]
        h2, st, bits2, m = emu.verify_batch(b.as_dict(), force_mode=mode)
        assert m == (mode - 4 if mode >= 5 else mode)
        bad = [f"{tags[i]} emu {st[i]} want {want[i]}" for i in np.flatnonzero(st != want)]
        assert not bad, (name, bad)
        assert np.array_equal(h2, h) and np.array_equal(bits2, bits), name


@pytest.mark.parametrize("mode", [2, 1, 5, 6])
def test_emulator_forged_triples_are_not_hashable(mode):
    """(The emulator hashes real bodies, so the forged triples cannot run in
    it: over bodies of the test's the same items must be REJECT, REF_PANIC,
    REJECT, REJECT — the order of the r / s checks and the key check.)"""
    from tests import chain_vectors as cv
    from tests.emu import emu

    vecs = kv.forged_items()
    b, _, _ = cv.batch(vecs)
    want = np.array([gs.REJECT if v.want == gs.ACCEPT else v.want for v in vecs], np.uint8)
    _, st, _, _ = emu.verify_batch(b.as_dict(), force_mode=mode)
    bad = [f"{vecs[i].tag} emu {st[i]} want {want[i]}" for i in np.flatnonzero(st != want)]
    assert not bad, bad


@pytest.fixture(scope="module")
def replay_exe():
    from tests import test_defer_exc as tde

    # tests/test_chain_exceptions.py's build
    return tde._build("chain", ["-DBV_DEFER_EXC=1", "-DBV_FUSED_Y3=1"], ["-O2"])


@pytest.mark.parametrize("geom", ["K12", "K8"])
def test_host_replay_of_the_forged_triples(replay_exe, tmp_path, geom):
    """tests/deferexc in its digests-in mode (key_decode_one, per-batch key
    tables built from the decoded limbs, verify_item_g + verify_item_q and the
    host entries' order): ACCEPT under every OK key — the decoded limbs of the
    extreme coordinates feed the table builders — REF_PANIC under the twins,
    REJECT where r or s is out of range."""
    from tests import test_chain_exceptions as tce

    vecs = kv.forged_items()
    want, rows = tce.replay(replay_exe, vecs, geom, tmp_path)
    bad = [f"{v.tag} device-order {t[2]} host-order {t[3]} want {w}" for v, w, t in zip(vecs, want, rows)
           if int(t[2]) != w or int(t[3]) != w]
    assert not bad, bad
