"""bench.py --dump-outputs on the CPU: the argument, and dump_messages over a made-up message list
(the GPU side -- that the files hold the last timed step -- is tests/test_gpu_parity.py)."""
import numpy as np
import pytest

import bench
from dump1090_rs_amd._lib import AdsbMsg


def fake_msgs(n, seed=5):
    rng = np.random.default_rng(seed)
    a = np.ctypeslib.as_array((AdsbMsg * n)()).copy()
    a["msg"] = rng.integers(0, 256, size=(n, 14))
    a["len"] = rng.choice([7, 14], size=n)
    a["try_phase"] = rng.integers(4, 9, size=n)
    a["score"] = rng.integers(-2000, 2000, size=n)
    a["j"] = rng.integers(0, 131072, size=n)
    a["chunk"] = np.sort(rng.integers(0, 1 << 40, size=n))
    a["signal_level"] = rng.random(n)
    return a


def test_dump_outputs_argument():
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"
    assert bench.parse([]).dump_outputs is None
    assert bench.parse(["--workload", "dense", "--dump-outputs", "d"]).dump_outputs == "d"
    for w in ("stream", "shard", "live"):
        with pytest.raises(SystemExit):
            bench.parse(["--workload", w, "--dump-outputs", "d"])


def test_dump_messages_writes_every_field_exactly(tmp_path):
    msgs = fake_msgs(300)
    info = bench.dump_messages(tmp_path / "out", msgs)
    assert (info["messages"], info["rows"]) == (300, 300)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in info["files"]}
    assert sorted(got) == ["chunk", "index", "j", "msg", "msglen", "score", "signal_level", "try_phase"]
    assert all(a.dtype in (np.float32, np.float64) and len(a) == 300 for a in got.values())
    assert info["bytes"] == sum(a.nbytes for a in got.values())
    assert np.array_equal(got["msg"].astype(np.uint8), msgs["msg"]) and got["msg"].shape == (300, 14)
    assert np.array_equal(got["msglen"], msgs["len"]) and np.array_equal(got["index"], np.arange(300))
    for f in ("try_phase", "score", "j", "chunk", "signal_level"):
        assert np.array_equal(got[f], msgs[f]), f
    assert bench.dump_messages(tmp_path / "empty", msgs[:0])["rows"] == 0


def test_dump_messages_samples_a_fixed_subset_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10_000)
    msgs = fake_msgs(1000)
    info = [bench.dump_messages(tmp_path / d, msgs) for d in ("a", "b")]
    assert info[0]["messages"] == 1000 and 0 < info[0]["rows"] < 1000 and info[0]["bytes"] <= 10_000
    a, b = ({f[:-4]: np.load(tmp_path / d / f) for f in i["files"]} for d, i in zip("ab", info))
    assert all(np.array_equal(a[f], b[f]) for f in a)                  # the same rows every time
    rows = a["index"].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a["chunk"], msgs["chunk"][rows])
