"""Item batches from signature text, the host side (CPU only): the header and
the bindings of bv_verify_batch_text / bv_decode_signatures, the batch decode
against the one-item parser (bv_decode_signature, itself fuzzed against the Go
restatement by tests/test_hostfuzz.py), its argument checks,
BatchBuilder.pack_text, and bv_decode_signatures under AddressSanitizer +
UBSan in a stand-alone program (tests/hostfuzz_text).  The device side is
tests/test_gpu_text_items.py."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from babble_amd import native, synth
from babble_amd.batch import BatchBuilder, PackedTextBatch
from tests.test_abi import declared_functions
from tests.test_hostfuzz import _sig_cases

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostfuzz_text")
EXE = os.path.join(HERE, "_build", "hostfuzz_text")
NEW = {"bv_verify_batch_text", "bv_decode_signatures"}


@pytest.fixture(scope="module")
def corpus():
    return _sig_cases(random.Random(7))


def _cat(texts):
    off = np.zeros(len(texts) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in texts])
    return off, np.frombuffer(b"".join(texts), np.uint8).copy()


def test_header_and_exports_declare_the_text_entries():
    assert NEW <= declared_functions() and NEW <= set(native.EXPORTS)
    L = native.lib()
    assert L.bv_abi_version() == native.ABI_VERSION == 6  # additive: the version stays
    for name in NEW:
        assert getattr(L, name).restype is ctypes.c_int
    # bv_text_batch: a bv_batch, then the two pointers
    assert native.BvTextBatch.items.offset == 0 and native.BvTextBatch.items.size == ctypes.sizeof(native.BvBatch)
    assert native.BvTextBatch.sig_off.offset == ctypes.sizeof(native.BvBatch)
    assert ctypes.sizeof(native.BvTextBatch) == ctypes.sizeof(native.BvBatch) + 16
    assert L.bv_verify_batch_text(None, None, None) == native.BV_E_ARGS


def test_decode_signatures_equals_one_item_calls(corpus):
    from tests.cabi import harness

    b = synth.blocks(5, 100, seed=21).batch  # 500 real signatures, as EncodeSignature writes them
    text, off = harness.encode_signatures(b.r_be, b.s_be)
    real = [harness.signature_text(text, off, i) for i in range(b.n_items)]
    texts = list(corpus) + real
    random.Random(3).shuffle(texts)
    toff, ttext = _cat(texts)
    pre, r, s = native.decode_signatures(toff, ttext)
    classes = set()
    for i, t in enumerate(texts):
        p1, r1, s1 = native.decode_signature(t)
        assert (int(pre[i]), r[i].tobytes(), s[i].tobytes()) == (p1, r1, s1), (i, t)
        if p1 == 0x80 or p1 & 3:  # zeros wherever a class is not OK
            assert r1 == bytes(32), t
        if p1 == 0x80 or p1 & 12:
            assert s1 == bytes(32), t
        classes.add(p1)
    assert {0, 0x80} <= classes and len(classes) > 8
    # the real ones decode back to the arrays they were written from
    back = native.decode_signatures(off, text)
    assert not back[0].any() and np.array_equal(back[1], b.r_be) and np.array_equal(back[2], b.s_be)


def test_decode_signatures_argument_checks():
    L = native.lib()
    off, text = _cat([b"1|2", b"3|4", b""])
    r, s, pre = np.zeros((3, 32), np.uint8), np.zeros((3, 32), np.uint8), np.zeros(3, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert L.bv_decode_signatures(3, p(off), p(text), p(r), p(s), p(pre)) == native.BV_OK
    assert pre.tolist() == [0, 0, 0x80] and r[0, 31] == 1 and s[1, 31] == 4
    down = np.array([0, 5, 3, 6], np.uint64)
    assert L.bv_decode_signatures(3, p(down), p(text), p(r), p(s), p(pre)) == native.BV_E_ARGS
    assert L.bv_decode_signatures(3, None, p(text), p(r), p(s), p(pre)) == native.BV_E_ARGS
    assert L.bv_decode_signatures(3, p(off), None, p(r), p(s), p(pre)) == native.BV_E_ARGS
    assert L.bv_decode_signatures(3, p(off), p(text), None, p(s), p(pre)) == native.BV_E_ARGS
    assert L.bv_decode_signatures(3, p(off), p(text), p(r), None, p(pre)) == native.BV_E_ARGS
    assert L.bv_decode_signatures(3, p(off), p(text), p(r), p(s), None) == native.BV_E_ARGS
    # nothing to decode: BV_OK, nothing read; only empty texts: no bytes needed
    assert L.bv_decode_signatures(0, None, None, None, None, None) == native.BV_OK
    zero = np.zeros(4, np.uint64)
    assert L.bv_decode_signatures(3, p(zero), None, p(r), p(s), p(pre)) == native.BV_OK
    assert pre.tolist() == [0x80] * 3 and not r.any() and not s.any()
    with pytest.raises(native.BvError):
        native.decode_signatures(down, text)
    with pytest.raises(native.BvError):
        native.decode_signatures(np.array([0, 3, 9], np.uint64), text)  # offsets past the text


def test_pack_text_round_trip(corpus):
    rng = random.Random(11)
    bb = BatchBuilder()
    msgs = [bb.add_msg(b"body %d" % i) for i in range(7)]
    keys = [bb.add_key(bytes([4, i]) * 10) for i in range(5)]
    sigs = [rng.choice(corpus) for _ in range(300)] + ["12|zz", "-1|+1", ""]
    for i, t in enumerate(sigs):
        assert bb.add_item(msgs[i % 7], keys[i % 5], t) == i
    pb, tb = bb.pack(), bb.pack_text()
    assert isinstance(tb, PackedTextBatch) and (tb.n_msgs, tb.n_keys, tb.n_items) == (7, 5, len(sigs))
    for f in ("msg_bytes", "msg_off", "key_bytes", "key_off", "item_msg", "item_key"):
        assert np.array_equal(getattr(tb, f), getattr(pb, f)), f
    assert tb.sig_off.dtype == np.uint64 and tb.sig_off[0] == 0 and tb.sig_off[-1] == tb.sig_text.size
    for i, t in enumerate(sigs):
        assert tb.signature(i) == (t.encode() if isinstance(t, str) else t)
    pre, r, s = native.decode_signatures(tb.sig_off, tb.sig_text)
    assert np.array_equal(pre, pb.pre) and np.array_equal(r, pb.r_be) and np.array_equal(s, pb.s_be)
    d = tb.decoded()
    assert np.array_equal(d.pre, pb.pre) and np.array_equal(d.r_be, pb.r_be) and np.array_equal(d.item_key, pb.item_key)
    # an item without its text cannot be packed as text; the raw pack still works
    bb.add_item_raw(msgs[0], keys[0], 0, bytes(32), bytes(32))
    with pytest.raises(ValueError):
        bb.pack_text()
    assert bb.pack().n_items == len(sigs) + 1
    empty = BatchBuilder().pack_text()
    assert empty.n_items == 0 and empty.sig_off.tolist() == [0] and empty.sig_text.size == 0


def test_decode_signatures_sanitized(corpus):
    """The stand-alone driver (its own main; nothing loaded into Python runs
    under a sanitizer): hostparse.cpp with -fsanitize=address,undefined."""
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    lines = [c.hex() or "-" for c in corpus]
    p = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    ok, batches, items = p.stdout.split()
    assert ok == "ok" and int(batches) > 400 and int(items) >= len(corpus) + 400
