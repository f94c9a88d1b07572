"""bench.py's command line: a plain run measures the headline alone, and --dump-outputs shows what it computed.

One plain run of the C5 stream mode at 20M events (20 events per key: about 8M matches, so the dump takes its sampling
path) is shared by the two GPU tests.  The line must carry the headline keys with `--steps` timed steps and none of the
measurements that `--full` adds; the dump must hold the last step's match records as float32 / float64 arrays within
64 MB, in delivery order, and each sampled record must satisfy the query it came from
(`e1=StockStream[price>20] -> e2=StockStream[price>e1.price]`: p2 > p1 > 20).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVENTS, STEPS = 20_000_000, 3

gpu = pytest.mark.gpu


def test_dump_records_decodes_and_samples(tmp_path, monkeypatch):
    """CPU check of the dump's record decoding and sampling: a host array in the layout of sg_match_records stands in
    for the engine's store (the device-to-device copy becomes a memmove), small budgets force several copy chunks and
    the sampling path.  Every written field must equal the record it was drawn from, nulls become NaN, and the same
    match count draws the same sample."""
    import ctypes as ct
    import types
    import torch
    import bench

    class FakeHip:
        @staticmethod
        def hipMemcpy(dst, src, n, kind):
            assert kind == 3
            ct.memmove(dst, src, n.value)
            return 0
    monkeypatch.setattr(bench, "ct", types.SimpleNamespace(CDLL=lambda name: FakeHip, c_void_p=ct.c_void_p,
                                                           c_size_t=ct.c_size_t))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    monkeypatch.setattr(bench, "DUMP_CHUNK", 70_001)
    nfa = types.SimpleNamespace(out_progs=[], out_types=[], select=[(0, 0, 0, "LONG"), (0, 0, 0, "DOUBLE"),
                                                                    (0, 0, 0, "FLOAT"), (0, 0, 0, "INT")])
    for n in (0, 5, 300_000):
        i = np.arange(n)
        rec = np.zeros((n, 8), np.int64)          # {u64 trigger; i64 ts; i32 key; u32 group; u32 vnull; u32 pad; vals[4]}
        w32 = rec.view(np.int32).reshape(n, 16)
        rec[:, 0], rec[:, 1] = i * 3, 1_700_000_000_000 + i
        w32[:, 4], w32[:, 5], w32[:, 6] = i % 1000 - 1, 0x01000002, (i % 7 == 0) * 4    # (column 2 null on every 7th)
        rec[:, 4] = i - 10
        rec[:, 5] = (i * 0.125).view(np.int64)
        w32[:, 12] = (i.astype(np.float32) * 0.5).view(np.int32)
        w32[:, 13] = -1                            # (the unused high half of a 4-byte value is never read)
        rec[:, 7] = -i
        m = types.SimpleNamespace(n=n, record_bytes=64, n_select=4, base=rec.ctypes.data)
        h = types.SimpleNamespace(device_records=lambda: m)
        out = tmp_path / ("n%d" % n)
        bench.dump_records(h, nfa, str(out), torch.device("cpu"))
        a = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
        ix = a["sample_index"].astype(np.int64)
        k = len(ix)
        assert a["matches"][0] == n and k == min(n, (1 << 20) // 80)
        assert np.all(np.diff(ix) > 0) and (k == 0 or (ix[0] >= 0 and ix[-1] < n))
        assert np.array_equal(a["trigger"], ix * 3) and np.array_equal(a["ts"], 1_700_000_000_000 + ix)
        assert np.array_equal(a["key"], ix % 1000 - 1) and np.all(a["group"] == 0x01000002)
        assert np.array_equal(a["vnull"], (ix % 7 == 0) * 4.0)
        assert np.array_equal(a["col0"], ix - 10) and np.array_equal(a["col1"], ix * 0.125)
        nul = ix % 7 == 0
        assert a["col2"].dtype == np.float32 and np.array_equal(np.isnan(a["col2"]), nul)
        assert np.array_equal(a["col2"][~nul], (ix.astype(np.float32) * 0.5)[~nul])
        assert np.array_equal(a["col3"], -ix)
        bench.dump_records(h, nfa, str(out) + "_again", torch.device("cpu"))
        assert np.array_equal(np.load(str(out) + "_again/sample_index.npy"), a["sample_index"])


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--c5-events", str(EVENTS), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), out


@gpu
def test_plain_line_is_the_headline_alone(plain_run):
    line, _ = plain_run
    assert line["unit"] == "events/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("events/sec")
    assert line["steps"] == STEPS and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    # value = the stream's events over one timed step (both are rounded in the line)
    assert line["value"] == pytest.approx(EVENTS / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["config"]["events_per_step"] == EVENTS
    assert line["whole_node"] is None and line["cpu_baseline"] is None and line["configs"] == {}
    assert line["roofline"]["kernel_ms"] > 0   # (from the timed steps' own HIP events)


@gpu
def test_dump_outputs_hold_the_last_steps_records(plain_run):
    line, out = plain_run
    names = sorted(f[:-4] for f in os.listdir(out) if f.endswith(".npy"))
    assert names == sorted(["matches", "sample_index", "trigger", "ts", "key", "group", "vnull",
                            "col0", "col1", "col2", "col3"])
    a = {n: np.load(os.path.join(out, n + ".npy")) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 << 20
    total = int(a["matches"][0])
    assert total == line["config"]["matches_per_step"] and total > 1_000_000
    k = len(a["sample_index"])
    assert 100_000 < k < total   # a sample: the records (72 B each as arrays) exceed the dump's budget
    assert all(len(a[n]) == k for n in names if n != "matches")
    idx = a["sample_index"]
    assert idx[0] >= 0 and idx[-1] < total and np.all(np.diff(idx) > 0)
    assert np.all(np.diff(a["trigger"]) >= 0)                        # delivery order: triggers never decrease
    assert a["trigger"].max() < EVENTS and np.all(a["vnull"] == 0)
    id1, id2, p1, p2 = (a["col%d" % j] for j in range(4))            # select e1.id, e2.id, e1.price, e2.price
    assert p1.dtype == np.float32 and p2.dtype == np.float32
    assert np.all(p1 > 20) and np.all(p2 > p1)
    assert np.all(id2 > id1) and np.all(id1 >= 0)                    # e2 arrives after e1
    assert np.array_equal(id2, a["trigger"])                         # the stream's id column is the event index
