"""The node pipeline (sg_node_*, siddhi_amd/csrc/node.hip) against the oracle: raw host rows -> native router
(first-seen dense ids, shard mix64(id) mod G) -> one thread per GPU with chunked H2D / kernels / D2H -> native merge
into the node's delivery order (PartitionStreamReceiver.receive(Event[]) feeding per-key runtimes and one ordered
QueryCallback stream, C/partition/PartitionStreamReceiver.java:177-221, C/partition/PartitionRuntime.java:255-308,
C/query/output/callback/QueryCallback.java:52-85).  G > 1 runs several shards on cuda:0 (one handle each)."""
import numpy as np
import pytest

from oracle import OracleEngine
from parity_util import assert_same, context, dense_first_seen, run_engine, synth_batch
from siddhi_amd import synth
from siddhi_amd.runtime import Batch, Outputs

pytestmark = pytest.mark.gpu

ABSENT_Q = ("@app:playback define stream S (id long, symbol string, v int, w int); "
            "partition with (symbol of S) begin @info(name='q') "
            "from every e1=S[v>700] -> not S[v<e1.v] for 30 milliseconds "
            "select e1.id as i1, e1.v as v1 insert into M; end;")


def node_outputs(nfa, sink, n):
    """Delivered SoA columns -> Outputs (vals as the bit patterns sg_poll reports)."""
    from siddhi_amd._native import column_dtypes
    dts = column_dtypes(nfa)
    vals = np.zeros((n, max(len(dts), 1)), np.int64)
    vnull = np.zeros((n, max(len(dts), 1)), np.uint8)
    for k, dt in enumerate(dts):
        c = sink.cols[k][:n]
        if np.dtype(dt) == np.float32:
            vals[:, k] = c.view(np.uint32).astype(np.int64)
        elif np.dtype(dt).itemsize == 4:
            vals[:, k] = c.view(np.int32).astype(np.int64)
        else:
            vals[:, k] = c.view(np.int64)
        vnull[:, k] = sink.nulls[k][:n]
    ns = len(dts)
    key = sink.key[:n].copy() if sink.key is not None else np.zeros(n, np.int32)   # (a sink without the key column)
    return Outputs(sink.trigger[:n].copy(), sink.ts[:n].copy(), key, sink.group[:n].copy(), vals[:, :ns], vnull[:, :ns])


def run_node(query, pushes, n_gpus, chunk_rows, raw_of, threads=4, cap=None, pinned=False, key_dict=0,
             fields=("trigger", "ts", "key", "group")):
    """Push host batches (their .key = synthetic key ids, sent as raw 64-bit symbols) through one node.  The returned
    stats carry the node's key count as st["keys"]."""
    from siddhi_amd import _native as N
    nfa = __import__("siddhi_amd.lowering", fromlist=["lower"]).lower(context(query))
    node = N.Node(N.build_desc(nfa), n_gpus=n_gpus, devices=[0] * n_gpus, threads=threads, chunk_rows=chunk_rows)
    if key_dict:
        node.set_key_dict(key_dict)
    outs = []
    for b in pushes:
        keep = []
        ts = np.ascontiguousarray(b.ts, np.int64)
        raw = np.ascontiguousarray(raw_of(b.key), np.int64)
        st = None if b.stream is None else np.ascontiguousarray(b.stream, np.int32)
        cols = [np.ascontiguousarray(c) for c in b.cols]
        nul = [None if x is None else np.ascontiguousarray(x, np.uint8) for x in b.nulls]
        keep += [ts, raw, st] + cols + nul
        nb = N.make_node_batch(b.n, b.base_index, ts.ctypes.data, 0 if st is None else st.ctypes.data,
                               raw.ctypes.data, [c.ctypes.data for c in cols],
                               [0 if x is None else x.ctypes.data for x in nul], keep)
        sink = N.ColumnSink(nfa, cap or (4 * b.n + 16), pinned=pinned, fields=fields)
        try:
            got = node.push(nb, sink.struct, sink.cap)
        except Exception:
            node.close()
            raise
        outs.append(node_outputs(nfa, sink, got))
    st = node.stats()
    st["keys"] = node.keys()
    node.close()
    return Outputs(*[np.concatenate([getattr(o, f) for o in outs]) for f in
                     ("trigger", "ts", "key", "group", "vals", "vnull")]), st


def _want(query, b):
    d = Batch(b.n, b.base_index, b.ts, b.stream, dense_first_seen(b.key), b.cols, b.nulls)
    return run_engine(OracleEngine, query, [d])


def _split(b, cuts):
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out.append(Batch(hi - lo, b.base_index + lo, b.ts[lo:hi], b.stream[lo:hi], b.key[lo:hi],
                         [c[lo:hi] for c in b.cols], [None if x is None else x[lo:hi] for x in b.nulls]))
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("key_dict", [1, 2], ids=["host-dict", "device-dict"])
@pytest.mark.parametrize("cfg,n,keys,rate,gpus,chunk", [
    ("C2", 200_000, 1_000, 100, 1, 30_000), ("C2", 200_000, 1_000, 100, 2, 45_000), ("C2", 200_000, 400, 100, 3, 0),
    ("C5", 300_000, 20_000, 1_000, 2, 70_000), ("C3b", 200_000, 400, 1_000, 2, 50_000),
    ("C3c", 200_000, 400, 100, 2, 60_000), ("C3c", 150_000, 400, 100, 1, 40_000)])
def test_node_matches_oracle(cfg, n, keys, rate, gpus, chunk, key_dict):
    b = synth_batch(cfg, 0, n, keys=keys, rate=rate)
    want = _want(synth.QUERIES[cfg], b)
    assert len(want) > 0
    got, st = run_node(synth.QUERIES[cfg], [b], gpus, chunk, synth.raw_symbols, key_dict=key_dict)
    assert st["matches"] == len(want)
    assert sum(st["shard_rows"][:gpus]) == n
    assert_same(got, want)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("key_dict", [1, 2], ids=["host-dict", "device-dict"])
@pytest.mark.parametrize("gpus", [1, 2])
def test_node_pushes_carry_state(gpus, key_dict):
    """Consecutive node pushes are one stream (per-key state and the key dictionary carry over)."""
    cfg = "C2"
    b = synth_batch(cfg, 0, 240_000, keys=800, rate=100)
    want = _want(synth.QUERIES[cfg], b)
    got, _ = run_node(synth.QUERIES[cfg], _split(b, [0, 50_000, 50_001, 170_000, 240_000]), gpus, 40_000,
                      synth.raw_symbols, key_dict=key_dict)
    assert_same(got, want)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gpus", [1, 2])
def test_node_device_dictionary_rebuild_and_sentinel(gpus):
    """The device dictionary (csrc/keydict.hip) at 2.5M keys: the first 4M-row chunk brings more new keys than half
    its initial 4M-slot table, so the table is rebuilt 4x larger and the chunk re-probed; one symbol's raw value is
    the table's empty-slot sentinel (INT64_MIN) and lives in the extra slot.  Keys get first-seen ids node-wide."""
    cfg = "C2"
    b = synth_batch(cfg, 0, 8_000_000, keys=3_000_000, rate=10_000)
    want = _want(synth.QUERIES[cfg], b)
    assert len(want) > 100_000

    def raw_of(k):
        r = synth.raw_symbols(k)
        return np.where(k == k[17], np.iinfo(np.int64).min, r)
    got, st = run_node(synth.QUERIES[cfg], [b], gpus, 4_000_000, raw_of, threads=8, key_dict=2)
    assert_same(got, want)


@pytest.mark.timeout(300)
def test_node_pinned_output_and_capacity():
    from siddhi_amd._native import SgError
    cfg = "C2"
    b = synth_batch(cfg, 0, 100_000, keys=500, rate=100)
    want = _want(synth.QUERIES[cfg], b)
    got, _ = run_node(synth.QUERIES[cfg], [b], 2, 30_000, synth.raw_symbols, pinned=True)
    assert_same(got, want)
    with pytest.raises(SgError) as ei:
        run_node(synth.QUERIES[cfg], [b], 1, 30_000, synth.raw_symbols, cap=len(want) // 2)
    assert ei.value.code == -3


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cfg,n", [("C1", 100_000), ("C4", 60_000)])
def test_node_unpartitioned_single_gpu(cfg, n):
    b = synth_batch(cfg, 0, n)
    want = run_engine(OracleEngine, synth.QUERIES[cfg], [b])
    got, _ = run_node(synth.QUERIES[cfg], [b], 1, 64_000, lambda k: np.zeros(len(k), np.int64))
    assert_same(got, want)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gpus", [1, 2, 3])
def test_node_partitioned_absence_clock_fanout(gpus):
    """Playback timers of every key fire on every row's clock: with G > 1 each shard gets clock rows for the rows
    it does not own, and timer emissions of one clock advance merge across shards by (phase, first-seen key)."""
    b = synth_batch("C3b", 0, 60_000, keys=200, rate=10)
    want = _want(ABSENT_Q, b)
    assert len(want) > 100
    got, _ = run_node(ABSENT_Q, [b], gpus, 25_000, synth.raw_symbols)
    assert_same(got, want)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gpus", [1, 2])
def test_node_ships_every_column_when_fill_is_off(gpus, monkeypatch):
    """SG_DEBUG_NODE_NO_FILL (a test hook): the closed form's trigger-row columns (ts, e2.*) come back from the GPU
    instead of being filled on the host from the batch -- both deliveries are the same rows."""
    monkeypatch.setenv("SG_DEBUG_NODE_NO_FILL", "1")
    cfg = "C2"
    b = synth_batch(cfg, 0, 150_000, keys=600, rate=100)
    want = _want(synth.QUERIES[cfg], b)
    got, _ = run_node(synth.QUERIES[cfg], [b], gpus, 40_000, synth.raw_symbols)
    assert_same(got, want)


def _first_seen_ids(keys, K):
    """Dense first-seen ids of keys in [0, K) without sorting the rows (the first occurrence wins the reversed
    fancy-index assignment)."""
    n = len(keys)
    first = np.full(K, n, np.int64)
    first[keys[::-1]] = np.arange(n - 1, -1, -1, dtype=np.int64)
    present = first < n
    order = np.argsort(first, kind="stable")
    ids = np.full(K, -1, np.int32)
    ids[order[:int(present.sum())]] = np.arange(int(present.sum()), dtype=np.int32)
    return ids[keys]


@pytest.mark.timeout(1100)
def test_node_c5_whole_1b_stream_ten_pushes():
    """BASELINE configs[4] in full: the whole 1B-event, 1M-key C5 stream as ten 100M-event node pushes over two
    shards on device 0 (raw symbols routed on the host, chunked H2D / kernels / D2H per shard, native merge; key
    dictionary and per-key partial matches carried between pushes), every delivered row compared with the oracle
    run key-sharded over the host cores with its engines -- and so its carried state -- kept across the same ten
    pushes (parity_util.CarriedShardedOracle).  The workers fork before the first push; the rows of each push are
    regenerated from the deterministic synth stream, so host memory stays at one push.

    The whole stream takes ~8 minutes on the box (profiles/r04/c5_whole_1b_test.log: 10 pushes, 399,303,893 matches, all
    equal); the default suite runs its first two pushes (200M events) and SG_C5_WHOLE=1 runs all ten."""
    import os
    from parity_util import CarriedShardedOracle
    from siddhi_amd import _native as N
    cfg = "C5"
    _, n, K, R = synth.CONFIGS[cfg]
    per = n // 10
    pushes = 10 if os.environ.get("SG_C5_WHOLE") == "1" else 2
    q = synth.QUERIES[cfg]
    oracle = CarriedShardedOracle(q, max(2, min(16, os.cpu_count() or 2)))
    nfa = __import__("siddhi_amd.lowering", fromlist=["lower"]).lower(context(q))
    node = N.Node(N.build_desc(nfa), n_gpus=2, devices=[0, 0], threads=16, chunk_rows=0)
    ids = np.full(K, -1, np.int64)   # first-seen dense id of every raw key so far (the node's dictionary order)
    nxt, total = 0, 0
    try:
        for p in range(pushes):
            lo = p * per
            g = synth.generate(cfg, lo, per, keys=K, rate=R)
            raw = synth.raw_symbols(g["key"])
            keep = []
            nb = N.make_node_batch(per, lo, g["ts"].ctypes.data, 0, raw.ctypes.data,
                                   [g["id"].ctypes.data, 0, g["price"].ctypes.data], [0, 0, 0], keep)
            sink = N.ColumnSink(nfa, per // 2, pinned=False)
            m = node.push(nb, sink.struct, sink.cap)
            got = node_outputs(nfa, sink, m)
            del sink, raw
            k64 = g["key"].astype(np.int64)
            uniq, first = np.unique(k64, return_index=True)
            new = ids[uniq] < 0
            order = np.argsort(first[new], kind="stable")
            ids[uniq[new][order]] = nxt + np.arange(int(new.sum()))
            nxt += int(new.sum())
            dense = ids[k64].astype(np.int32)
            b = Batch(per, lo, g["ts"], np.zeros(per, np.int32), dense, [g["id"], g["key"], g["price"]], [None] * 3)
            want = oracle.push(b)
            del g, b, dense, k64
            assert len(got) == len(want) > 0, (p, len(got), len(want))
            assert_same(got, want)
            total += len(got)
            print(f"push {p}: {len(got)} matches equal the oracle's", flush=True)   # (progress: a long test)
            del got, want
        assert node.keys() == K == nxt
    finally:
        oracle.close()
        node.close()
    assert total > 36_000_000 * pushes


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ts32", [True, False])
def test_node_timestamp_offsets_and_wide_chunks(ts32, monkeypatch):
    """Chunk timestamps travel as 32-bit offsets from the chunk's minimum; a chunk spanning 2^31 ms or more (here a
    35-day gap in the middle of the stream) ships them as 8 bytes.  SG_DEBUG_NODE_NO_TS32 (a test hook) forces 8 bytes
    everywhere.  (With two GPUs the rows travel as they are: the shard exchange uploads 8-byte timestamps.)"""
    if not ts32:
        monkeypatch.setenv("SG_DEBUG_NODE_NO_TS32", "1")
    cfg = "C2"
    b = synth_batch(cfg, 0, 200_000, keys=700, rate=100)
    b.ts = b.ts.copy()
    b.ts[90_000:] += 3_000_000_000
    want = _want(synth.QUERIES[cfg], b)
    for gpus in (1, 2):
        got, _ = run_node(synth.QUERIES[cfg], [b], gpus, 40_000, synth.raw_symbols)
        assert_same(got, want)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gpus", [1, 2])
def test_node_carried_rows_reach_back_across_pushes(gpus):
    """Key X is quiet from row 1000 to row 80000 (10..800 ms), so its early rows are carried through four pushes and
    complete matches in the fifth: e1's columns come from the carried rows, on one GPU and through the exchange."""
    cfg = "C2"
    b = synth_batch(cfg, 0, 160_000, keys=600, rate=100)
    b.key = b.key.copy()
    x = b.key[3]
    quiet = np.arange(1000, 80_000)
    b.key[quiet[b.key[quiet] == x]] = (x + 1) % 600
    b.cols[1] = b.key
    want = _want(synth.QUERIES[cfg], b)
    assert np.any((want.trigger >= 80_000) & (want.vals[:, 0] < 1000))   # e1 rows from the first push, matched in the fifth
    got, _ = run_node(synth.QUERIES[cfg], _split(b, [0, 20_000, 40_000, 60_000, 80_000, 160_000]), gpus, 30_000,
                      synth.raw_symbols)
    assert_same(got, want)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gpus", [2, 3, 4, 8])
def test_node_shard_exchange(gpus):
    """The GPU-side shard exchange with G shards on cuda:0: slices of uneven size, chunks whose slices send no row to
    some shard (few keys), a two-stream partitioned query (PP), and the host's per-chunk work only: route_ms and
    merge_ms stay at zero."""
    for cfg, n, keys, rate, chunk in (("C2", 150_000, 5, 100, 17_001), ("PP", 120_000, 300, 100, 25_000),
                                      ("C3c", 100_000, 200, 100, 33_333)):
        b = synth_batch(cfg, 0, n, keys=keys, rate=rate)
        want = _want(synth.QUERIES[cfg], b)
        assert len(want) > 0
        got, st = run_node(synth.QUERIES[cfg], [b], gpus, chunk, synth.raw_symbols, key_dict=2)
        assert_same(got, want)
        assert st["route_ms"] == 0 and st["merge_ms"] == 0
        assert sum(st["shard_rows"][:gpus]) == n


# ---- the exchange's branches that the sizes above never reach: tiny inputs, each a few chunks of a few rows ----------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("cfg,gpus,chunk", [("C2", 8, 5), ("PP", 3, 7), ("C3c", 3, 7)])
def test_node_exchange_empty_slices_shards_and_chunks(cfg, gpus, chunk):
    """400 rows of 7 keys in chunks of 5 rows over 8 GPUs: every chunk has slices of zero rows (no shard count is
    launched for them), the 7 keys reach only 3 of the 8 shards (the others never resolve or push a row) and 24 of the
    80 chunks hold no trigger (no shard has matches, no owner merges).  PP and C3c the same way over 3 GPUs."""
    n = 400
    b = synth_batch(cfg, 0, n, keys=7, rate=100)
    want = _want(synth.QUERIES[cfg], b)
    assert len(want) > 0
    got, st = run_node(synth.QUERIES[cfg], [b], gpus, chunk, synth.raw_symbols, key_dict=2)
    assert_same(got, want)
    assert st["chunks"] == -(-n // chunk)
    assert sum(st["shard_rows"][:gpus]) == n
    assert st["route_ms"] == 0 and st["merge_ms"] == 0


@pytest.mark.timeout(300)
def test_node_exchange_fewer_rows_than_gpus():
    b = synth_batch("C2", 0, 5, keys=2)
    want = _want(synth.QUERIES["C2"], b)
    assert len(want) == 2
    got, st = run_node(synth.QUERIES["C2"], [b], 8, 0, synth.raw_symbols, key_dict=2)
    assert_same(got, want)
    assert sum(st["shard_rows"][:8]) == 5


@pytest.mark.timeout(300)
@pytest.mark.parametrize("chunk", [1000, 100])
def test_node_exchange_key_table_grows_across_chunks_and_pushes(chunk):
    """2,578 distinct keys over two shards in two pushes: each GPU's table of node-wide key ids (local id -> first-seen
    id) is appended to chunk after chunk and push after push.  It is allocated for 1.5 x the first chunk's keys + 1024:
    with 1000-row chunks that holds a shard's ~1,290 keys to the end; with 100-row chunks (~50 keys per shard in the
    first) the table is outgrown and copied into a larger one."""
    cfg = "C2"
    b = synth_batch(cfg, 0, 6000, keys=3000, rate=100)
    want = _want(synth.QUERIES[cfg], b)
    assert len(want) > 0
    got, st = run_node(synth.QUERIES[cfg], _split(b, [0, 2500, 6000]), 2, chunk, synth.raw_symbols, key_dict=2)
    assert_same(got, want)   # (keys: the oracle's first-seen ids)
    assert st["keys"] == len(np.unique(b.key))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gpus", [2, 4])
def test_node_exchange_without_key_column(gpus):
    """A sink without the key column: the exchange skips the node-wide key ids altogether."""
    cfg = "C2"
    b = synth_batch(cfg, 0, 400, keys=7, rate=100)
    want = _want(synth.QUERIES[cfg], b)
    assert len(want) > 0
    got, _ = run_node(synth.QUERIES[cfg], [b], gpus, 60, synth.raw_symbols, key_dict=2,
                      fields=("trigger", "ts", "group"))
    assert len(got) == len(want)
    for f in ("trigger", "ts", "group", "vnull"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert np.array_equal(np.where(got.vnull.astype(bool), 0, got.vals), np.where(want.vnull.astype(bool), 0, want.vals))


@pytest.mark.timeout(300)
def test_node_exchange_capacity_error():
    """More matches than the output capacity, through the exchange: every GPU's loop ends (none is left waiting for a
    step the others gave up) and the push reports SG_ECAPACITY; a fresh node with room delivers the oracle's rows."""
    from siddhi_amd._native import SgError
    cfg = "C2"
    b = synth_batch(cfg, 0, 400, keys=7, rate=100)
    want = _want(synth.QUERIES[cfg], b)
    assert len(want) > 80
    with pytest.raises(SgError) as ei:
        run_node(synth.QUERIES[cfg], [b], 2, 100, synth.raw_symbols, key_dict=2, cap=80)
    assert ei.value.code == -3
    got, _ = run_node(synth.QUERIES[cfg], [b], 2, 100, synth.raw_symbols, key_dict=2)
    assert_same(got, want)
