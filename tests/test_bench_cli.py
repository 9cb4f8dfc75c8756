"""bench.py's command line: a plain run is the headline alone, `--full` turns
the other legs on, `--dump-outputs` writes exact float copies of a result."""
import numpy as np

import bench
from babble_amd.verifier import VerifyResult


def _parse(monkeypatch, argv):
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_headline_only(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup) == (7, 3)
    assert not a.full and a.no_cpu and a.no_extras and a.dump_outputs is None


def test_full_turns_the_legs_on(monkeypatch):
    a = _parse(monkeypatch, ["--full"])
    assert a.full and not a.no_cpu and not a.no_extras
    a = _parse(monkeypatch, ["--full", "--no-cpu", "--no-extras"])
    assert a.full and a.no_cpu and a.no_extras


def test_dump_outputs_is_exact_and_bounded(tmp_path):
    rng = np.random.default_rng(1)
    n = bench.DUMP_HASH_ROWS + 1000  # more messages than the sample holds
    res = VerifyResult(rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 4, n, dtype=np.uint8),
                       rng.integers(0, 2**64, (n + 63) // 64, dtype=np.uint64))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert set(got) == {"status", "accept_bits_u32", "msg_hash", "msg_hash_rows"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["status"].astype(np.uint8), res.status)
    assert np.array_equal(got["accept_bits_u32"].astype(np.uint32).view(np.uint64), res.accept_bits)
    rows = got["msg_hash_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_HASH_ROWS and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert np.array_equal(got["msg_hash"].astype(np.uint8), res.msg_hash[rows])
    for name, a in got.items():  # the same rows and values from call to call
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))
    # the headline workload (1M items, 1M messages) stays far below 64 MB
    assert 4 * 10**6 + 8 * 2 * 15625 + bench.DUMP_HASH_ROWS * (32 * 4 + 8) < 64 * 2**20
