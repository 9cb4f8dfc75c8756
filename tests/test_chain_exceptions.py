"""The valid exceptional-addition vectors of tests/chain_vectors.py on the CPU:
the crafting invariants, the expected statuses against
oracle.gosemantics.item_status over the supplied digests, and the evidence
that every vector meets the addition it targets.

For the per-lane key-table chains that evidence is a replay of the kernels'
own source: tests/deferexc/deferexc_main.cpp in its digests-in mode, built
with BV_DEFER_EXC=1, runs verify_item_g + verify_item_q<K12 | K8> and
verify_item_gq_kc<KC22 | KC18> (over sparse cached tables) on the host; by
the lemma in verify_core.h an item takes the second pass exactly when some
addition had P == 0, so every crafted vector must be flagged and no plain
valid vector may be.  The host entries' order (verify_item_qfirst +
verify_item_gfinish, all four key-table geometries) is replayed the same way
in a second build that keeps the product's 26-bit generator windows, which
host_vectors target, over a sparse generator table; there verify_item_gfinish
must be the call that is flagged.  The generic path and k_small have no host
build (coop.h is device-only), so for them the evidence is the order model of
chain_vectors, whose small-kernel constants are read from kernels.hip: in
Python integers the modelled operands are equal or opposite at the targeted
step and at no other.  That is the limit of this test: a chain whose real
order differs from its model would leave those vectors valid but vacuous."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import gosemantics as gs
from tests import chain_vectors as cv
from tests import edge_vectors as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "babble_amd", "csrc")
N = cv.N

FAMILIES = {
    "K12": lambda: cv.k_vectors("K12"), "K8": lambda: cv.k_vectors("K8"), "KC22": lambda: cv.k_vectors("KC22"),
    "KC18": lambda: cv.k_vectors("KC18"), "generic": cv.generic_vectors, "cold": cv.cold_vectors,
    "warmKC22": lambda: cv.warm_vectors("KC22"), "warmKC18": lambda: cv.warm_vectors("KC18"), "host": cv.host_vectors,
}
# (vectors, of which REJECT: the total is the identity)
COUNTS = {"K12": (24, 2), "K8": (24, 2), "KC22": (24, 2), "KC18": (24, 2), "generic": (12, 2), "cold": (18, 2),
          "warmKC22": (8, 1), "warmKC18": (10, 1), "host": (12, 2)}


def model(family, v):
    """every addition chain the family's path runs for v: {name: steps}"""
    if family in cv.K_GEOMETRIES:
        return {"q": cv.k_steps(v, geom=family)}
    if family == "generic":
        return {"g": cv.generic_steps(v.u1, v.u2, v.c)}
    if family == "cold":
        return cv.cold_chains(v.u1, v.u2, v.c)
    if family == "host":  # the host-entry order under each of the four key-table geometries
        return {geom: cv.host_steps(v.u1, v.u2, v.c, geom) for geom in cv.K_GEOMETRIES}
    return cv.warm_chains(v.u1, v.u2, v.c, family[4:])


def expected_collisions(family, v):
    if v.target is None:
        return []
    if family in cv.K_GEOMETRIES:
        return [("q", v.target, v.sign)]
    if family == "generic":
        return [("g", v.target, v.sign)]
    if family == "host":
        return sorted((geom, v.target, v.sign) for geom in cv.K_GEOMETRIES)
    return [(v.target[0], v.target[1], v.sign)]


def test_geometry_and_schedule_constants_match_the_source():
    geo = open(os.path.join(CSRC, "geometry.h")).read()

    def macro(name):
        return int(re.search(r"#define %s (\d+)" % name, geo).group(1))

    assert (macro("BV_GW"), macro("BV_GNWIN")) == (cv.GW, cv.GNWIN)
    assert (macro("BV_K12W"), macro("BV_K12NWIN")) == cv.K_GEOMETRIES["K12"][:2]
    assert (macro("BV_KW"), macro("BV_KNWIN")) == cv.K_GEOMETRIES["K8"][:2]
    assert (macro("BV_KCW"), macro("BV_KCNWIN")) == cv.K_GEOMETRIES["KC22"][:2] == cv.WARM_GEOMETRIES["KC22"][:2]
    assert (macro("BV_KC18W"), macro("BV_KC18NWIN")) == cv.K_GEOMETRIES["KC18"][:2] == cv.WARM_GEOMETRIES["KC18"][:2]
    k = cv.small_constants()
    assert k["kColdBudget"] >= 2 and k["kColdChunk"] >= 1 and k["kColdPre"] >= 1
    for geom, split in k["kWarmSplit"].items():
        assert split[0] == 0 and split == sorted(split) and len(set(split)) == 5, (geom, split)
        # the targets below exist only while some wave's range starts in the generator pairs and ends in key pairs
        assert cv.warm_targets(geom)[:-2], geom


@pytest.mark.parametrize("family", list(FAMILIES))
def test_vectors_are_valid_and_meet_their_target(family):
    """No vector dropped; r != 0, 0 < s <= (N - 1) / 2; the digest gives back
    the chosen u1, u2; the status over that digest is ACCEPT unless the total
    is the identity; and in the family's order model the accumulator equals
    the entry or its opposite at the targeted step and at no other."""
    vecs = FAMILIES[family]()
    n, n_reject = COUNTS[family]
    assert len(vecs) == n and len({v.tag for v in vecs}) == n
    assert sum(v.want == gs.REJECT for v in vecs) == n_reject
    for v in vecs:
        assert v.r % N and 0 < v.s <= (N - 1) // 2, v.tag
        w = pow(v.s, -1, N)
        e = int.from_bytes(v.digest, "big")
        assert e < N and e * w % N == v.u1 and v.r * w % N == v.u2 and v.u1 and v.u2, v.tag
        assert gs.item_status(v.pub, v.digest, v.r, v.s) == v.want, v.tag
        assert (v.want == gs.REJECT) == (v.total == 0), v.tag
        assert cv.all_collisions(model(family, v)) == expected_collisions(family, v), v.tag
    crafted = [v for v in vecs if v.target is not None]
    assert {v.sign for v in crafted} == {1, -1}


def test_host_vectors_reach_the_final_generator_window():
    """On each key the "last" target is the top generator window, the FINAL
    (xz_only) addition of verify_item_gfinish, met both ways; the others are
    window 0 (a non-identity accumulator entering it) and one in between."""
    by_key = {}
    for v in cv.host_vectors():
        by_key.setdefault(v.c, []).append(v)
    assert len(by_key) == 2 and set(by_key) == {v.c for v in cv.k_vectors("K12")}
    for vecs in by_key.values():
        assert {(v.target, v.sign) for v in vecs} >= {(("g", cv.GNWIN - 1), 1), (("g", cv.GNWIN - 1), -1)}
        assert len({v.target for v in vecs}) == 3 and all(v.target[0] == "g" for v in vecs)
        assert min(v.target[1] for v in vecs) == 0


def test_host_invalid_twins_share_the_chain_and_do_not_verify():
    """The twins of host_vectors: the digest gives back the SAME u1, u2 (so
    the same chain and collision under every geometry), r, s keep the
    conventions, and the status over that digest is REJECT for all 12."""
    twins, src = cv.host_invalid_twins(), cv.host_vectors()
    assert len(twins) == len(src) == 12 and len({v.tag for v in twins}) == 12
    for t, v in zip(twins, src):
        assert t.r % N and 0 < t.s <= (N - 1) // 2 and (t.r, t.s) != (v.r, v.s), t.tag
        w = pow(t.s, -1, N)
        assert (int.from_bytes(t.digest, "big") * w % N, t.r * w % N, t.pub) == (v.u1, v.u2, v.pub), t.tag
        assert t.want == gs.REJECT == gs.item_status(t.pub, t.digest, t.r, t.s), t.tag
        assert cv.all_collisions(model("host", t)) == expected_collisions("host", v), t.tag


def test_plain_fillers_meet_nothing():
    """The filler / control vectors collide nowhere, in any model."""
    for i, v in enumerate(cv.plain(0xF111, 4)):
        assert v.want == gs.ACCEPT == gs.item_status(v.pub, v.digest, v.r, v.s)
        for family in FAMILIES:
            assert cv.all_collisions(model(family, v)) == [], (i, family)


def test_identity_node_vectors_hand_over_identity_nodes():
    """the warm tree's identity-node vectors do have leaf pairs of two zero
    digits, among the generator pairs and among the key pairs"""
    for geom in cv.WARM_GEOMETRIES:
        for v in cv.warm_vectors(geom)[-2:]:
            chains = cv.warm_chains(v.u1, v.u2, v.c, geom)
            zero = [int(name[4:]) for name, steps in chains.items()
                    if name.startswith("pair") and all(x == 0 for _, x in steps)]
            assert any(i < cv.GNWIN // 2 for i in zero) and any(i >= cv.GNWIN // 2 for i in zero), (v.tag, zero)
            assert any(x for name, steps in chains.items() if name.startswith("pair") for _, x in steps)


@pytest.fixture(scope="module")
def replay_exe():
    from tests import test_defer_exc as tde

    # a build directory of this module's own (tests/deferexc/_build/chain)
    return tde._build("chain", ["-DBV_DEFER_EXC=1", "-DBV_FUSED_Y3=1"], ["-O2"])


def cached_slots(vecs, batch, geom):
    """The entries of the cached tables that the items' lookups add, as lines
    "<key> <slot> <x> <y>": window j of either GLV half reads slot
    j 2^(W-1) + |d| of the key's ONE stored half, which holds |d| 2^(W j) Q
    (phi is formed per lookup)."""
    w, nwin, _ = cv.K_GEOMETRIES[geom]
    kidx = {batch.key(k): k for k in range(batch.n_keys)}
    lines = {}
    for v in vecs:
        for k in ev.glv_halves(v.u2):
            for j, d in enumerate(ev.signed_digits(abs(k), w, nwin)):
                key = (kidx[v.pub], j * (1 << (w - 1)) + abs(d))
                if d and key not in lines:
                    x, y = gs.scalar_mult((abs(d) << (w * j)) * v.c % N, gs.G)
                    lines[key] = f"{key[0]} {key[1]} {x:064x} {y:064x}"
    return "\n".join(lines.values()) + "\n"


def g_slots(vecs):
    """The entries of the generator table (the product's 26-bit x 10 signed
    windows) that the items' u1 add, as lines "<slot> <x> <y>": window j reads
    slot j 2^25 + |d|, which holds |d| 2^(26 j) G."""
    lines = {}
    for v in vecs:
        for j, d in enumerate(ev.signed_digits(v.u1, cv.GW, cv.GNWIN)):
            slot = j * (1 << (cv.GW - 1)) + abs(d)
            if d and slot not in lines:
                x, y = gs.scalar_mult((abs(d) << (cv.GW * j)) % N, gs.G)
                lines[slot] = f"{slot} {x:064x} {y:064x}"
    return "\n".join(lines.values()) + "\n"


def replay(exe, vecs, geom, tmp_path, sparse_g=False):
    """(expected statuses, the program's rows) of the vectors through
    tests/deferexc in its digests-in mode for `geom`."""
    from tests.emu import emu

    b, dig, want = cv.batch(vecs)
    path, dpath = str(tmp_path / "batch.bin"), str(tmp_path / "digests.bin")
    emu.dump_batch(path, b.as_dict())
    dig.tofile(dpath)
    args = [exe, path, "8", dpath, geom.lstrip("KC")]
    if geom.startswith("KC"):
        spath = str(tmp_path / "slots.txt")
        with open(spath, "w") as f:
            f.write(cached_slots(vecs, b, geom))
        args.append(spath)
    elif sparse_g:
        args.append("-")
    if sparse_g:
        gpath = str(tmp_path / "gslots.txt")
        with open(gpath, "w") as f:
            f.write(g_slots(vecs))
        args.append(gpath)
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, env={"PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines()[1:]]
    assert len(rows) == len(vecs)
    return want, rows


@pytest.mark.parametrize("geom", ["K12", "K8", "KC22", "KC18"])
def test_host_replay_flags_every_crafted_vector(replay_exe, tmp_path, geom):
    """The per-lane chains compiled for the host with BV_DEFER_EXC=1, over the
    supplied digests: verify_item_g + verify_item_q<K12 | K8>, and
    verify_item_gq_kc<22, 6 | 18, 8> over sparse cached tables that hold the
    entries the items read.  The statuses are the expected ones, every
    crafted vector takes the second pass (ZZ == 0 after the unchecked chain:
    some addition had P == 0) and the plain valid vectors do not; the
    generator chain of verify_item_g is never flagged.  In the host entries'
    order (verify_item_qfirst + verify_item_gfinish over the same tables)
    the valid ones among these vectors are plain: the expected statuses and
    no second pass in either call, except verify_item_gfinish's for the two
    whose total is the identity, which every order meets in its last
    addition."""
    crafted = cv.k_vectors(geom)
    vecs = crafted + cv.plain(0xF111, 4, crafted[0].c)
    want, rows = replay(replay_exe, vecs, geom, tmp_path)
    for v, w, t in zip(vecs, want, rows):
        st_dev, st_host, redo_g, redo_q, redo_qf, redo_gf = (int(x) for x in t[2:8])
        assert st_dev == w, (v.tag, st_dev, w)
        assert redo_g == 0, v.tag
        assert redo_q == (1 if v.target is not None else 0), (v.tag, redo_q)
        assert st_host == w, (v.tag, st_host, w)
        # (a total of zero is P + (-P) at the last non-zero addition of ANY order: the 2 REJECT vectors)
        assert redo_qf == 0 and redo_gf == (1 if v.total == 0 else 0), (v.tag, redo_qf, redo_gf)
    assert np.count_nonzero(want == gs.ACCEPT) == len(vecs) - 2


@pytest.fixture(scope="module")
def host_replay_exe():
    from tests import test_defer_exc as tde

    # The product's generator geometry (geometry.h's 26-bit x 10 windows, which
    # host_vectors target) in place of the emulator's 16-bit one: the table is
    # then a sparse one (g_slots), since no host holds its 21.5 GB.
    product_g = ["-UBV_GW", "-UBV_GNWIN", "-UBV_GL", "-UBV_GNSUB"]
    return tde._build("chainhost", product_g + ["-DBV_DEFER_EXC=1", "-DBV_FUSED_Y3=1"], ["-O2"])


@pytest.mark.parametrize("geom", ["K12", "K8", "KC22", "KC18"])
def test_host_order_replay_flags_every_crafted_vector(host_replay_exe, tmp_path, geom):
    """The host entries' order compiled for the host with BV_DEFER_EXC=1 and
    the product's generator windows: verify_item_qfirst<geom> from the
    identity, then verify_item_gfinish — g_table_add<..., FROM_INF = false,
    FINAL = true, DEFER> onto R_Q, its top window the trimmed addition, its
    redo restarting from R_Q in memory.  Over host_vectors and plain fillers on
    both keys: the expected statuses (a wrong redo turns an ACCEPT into a
    REJECT); verify_item_gfinish takes the second pass for every crafted
    vector and for no filler; verify_item_qfirst never does (its chain starts
    at the identity and these u2 meet nothing: the lemma at BV_DEFER_EXC).
    host_invalid_twins run the same chains under signatures that do not
    verify: flagged alike, and REJECT — a flagged item that is not redone
    ends on X = ZZ = 0 and would ACCEPT, whatever r is, so the valid vectors
    alone cannot show a missing redo.  The device order of the same build
    must decide the same."""
    crafted = cv.host_vectors() + cv.host_invalid_twins()
    vecs = crafted + [p for c in sorted({v.c for v in crafted}) for p in cv.plain(0xF111, 2, c)]
    want, rows = replay(host_replay_exe, vecs, geom, tmp_path, sparse_g=True)
    for v, w, t in zip(vecs, want, rows):
        st_dev, st_host, redo_qf, redo_gf = int(t[2]), int(t[3]), int(t[6]), int(t[7])
        assert st_host == w, (v.tag, st_host, w)
        assert redo_gf == (1 if v.target is not None else 0), (v.tag, redo_gf)
        assert redo_qf == 0, v.tag
        assert st_dev == w, (v.tag, st_dev, w)
    assert np.count_nonzero(want == gs.ACCEPT) == 10 + 4  # host_vectors' ACCEPTs and the fillers


def _body(src, head):
    """the body of the function whose definition starts with `head`, comments
    and white space removed"""
    at = src.index(head)
    end = src.index("\n}\n", at)
    text = re.sub(r"//[^\n]*", "", src[src.index("{", at) + 1:end])
    return re.sub(r"\s+", "", text)


def test_bulk_entry_is_still_the_product_device_entry():
    """tests/chaincheck's bulk_impl is verify_device_impl (bv_api.cpp) with
    the digests copied in and `hashed` set: compared here text for text, so
    a change to the product's entry shows up instead of letting the copy
    drift."""
    api = open(os.path.join(CSRC, "bv_api.cpp")).read()
    cc = open(os.path.join(ROOT, "tests", "chaincheck", "chaincheck.hip")).read()
    product = _body(api, "static int verify_device_impl(bv_ctx *ctx, const bv_batch *dbatch, bv_result *dresult, "
                         "hipStream_t st) {")
    copy = _body(cc, "int bulk_impl(")
    a, z = copy.index("constuint64_tn_msgs=dbatch->n_msgs;"), copy.index("returnbv_run_device(")
    assert "S().digests" in copy[a:z]
    copy = copy[:a] + copy[z:]
    assert copy.count("st,true,kc);") == 1
    assert copy.replace("st,true,kc);", "st,false,kc);") == product


def test_host_order_entry_is_still_the_product_host_entry():
    """tests/chaincheck's hostorder_impl makes bv_host_launch's calls (bv_api.cpp)
    in bv_host_launch's order: bv_run_keys without the s^-1 stream's GLV split,
    the pipe over the call's stream, the context's own output buffers with
    `hashed` digests, the key part on the s^-1 stream, chunks, finish — the
    staging, hashing and copies between them aside.  A change to the product's
    sequence shows up here instead of leaving the test entry on the old one."""
    api = open(os.path.join(CSRC, "bv_api.cpp")).read()
    cc = open(os.path.join(ROOT, "tests", "chaincheck", "chaincheck.hip")).read()
    product = _body(api, "int bv_host_launch(bv_ctx *ctx, const bv_batch *b, bv_host_call *call, const bv_result *res,")
    copy = _body(cc, "int hostorder_impl(")
    calls = re.compile(r"bv_run_keys\(|bv_run_device\(|bv_run_verify\(|bv_launch_items\(|bv_item_pipepipe\{|"
                       r"bv_out_bufs\(|pipe\.key_part\(|pipe\.upto\(|pipe\.finish\(")
    want = ["bv_run_keys(", "bv_item_pipepipe{", "bv_out_bufs(", "pipe.key_part(", "pipe.upto(", "pipe.finish("]
    for name, text in (("bv_host_launch", product), ("hostorder_impl", copy)):
        assert calls.findall(text) == want, name
        assert len(re.findall(r"bv_run_keys\(ctx,&?\w+,[^;]*?,kc,false[,)]", text)) == 1, name  # split_ok = false
        assert len(re.findall(r"bv_item_pipepipe\{ctx,&?\w+,\{\},st,kc\};", text)) == 1, name
        assert text.count("nullptr,nullptr,nullptr,true,&pipe.o);") == 1, name  # hashed = true
        assert text.count("pipe.key_part(ctx->sstream,") == 1, name
        assert "hipStream_tst=ctx->stream" in text or name == "hostorder_impl"
    # the copy's caller hands it ctx->stream, where bv_host_launch runs
    caller = _body(cc, "int cc_verify_hostorder(")
    assert "hipStream_tst=ctx->stream;" in caller and "hostorder_impl(ctx,dbatch,dresult,d_digests,st," in caller
