"""Range partitions through the node pipeline (sg_node_set_ranges, siddhi_amd/csrc/node.hip): raw rows of a
range-partitioned stream go in, the GPUs hold, count and scatter one copy per holding range to the shard of its label,
and the delivered matches carry the event index of the row that completed them, in the written order of the ranges.

Every expectation is the oracle engine over range_ref.route's copies (node_range_cases.py; test_node_range_cases.py
guards the cases on the CPU).  G > 1 runs several shards on device 0 (one handle each)."""
import numpy as np
import pytest

import node_range_cases as NC
from parity_util import assert_same
from siddhi_amd.runtime import Outputs
from test_node import node_outputs

pytestmark = pytest.mark.gpu

SG_EINVAL, SG_EUNSUPPORTED = -1, -4


def open_node(p: NC.Prepared, gpus, chunk_rows=0, ranges=True):
    from siddhi_amd import _native as N
    node = N.Node(N.build_desc(p.nfa), n_gpus=gpus, devices=[0] * gpus, threads=4, chunk_rows=chunk_rows)
    if ranges:
        node.set_ranges(N.build_range_desc(p.table), p.label_raw)
    return node


def push(node, p: NC.Prepared, lo, hi, fields=("trigger", "ts", "key", "group"), base=None):
    """rows [lo, hi) of the case as one sg_node_push: the delivered Outputs"""
    from siddhi_amd import _native as N
    b, c = p.batch, p.case
    keep = []
    ts = np.ascontiguousarray(b.ts[lo:hi], np.int64)
    raw = np.ascontiguousarray(p.raw_key[lo:hi], np.int64)
    st = None if c.no_stream else np.ascontiguousarray(b.stream[lo:hi], np.int32)
    cols = [np.ascontiguousarray(x[lo:hi]) for x in b.cols]
    nul = [None if x is None else np.ascontiguousarray(x[lo:hi], np.uint8) for x in b.nulls]
    keep += [ts, raw, st] + cols + nul
    nb = N.make_node_batch(hi - lo, c.base + lo if base is None else base, ts.ctypes.data,
                           0 if st is None else st.ctypes.data, raw.ctypes.data, [x.ctypes.data for x in cols],
                           [0 if x is None else x.ctypes.data for x in nul], keep)
    sink = N.ColumnSink(p.nfa, c.cap_per_row * (hi - lo) + 64, pinned=False, fields=fields)
    got = node.push(nb, sink.struct, sink.cap)
    return node_outputs(p.nfa, sink, got)


def run_case(name, gpus, chunk_rows=0, fields=("trigger", "ts", "key", "group")):
    """the case through one node: (delivered Outputs, node stats, range stats, the prepared case)"""
    p = NC.prepared(name)
    node = open_node(p, gpus, chunk_rows)
    try:
        outs = [push(node, p, lo, hi, fields) for lo, hi in NC.pieces(p)]
        st, rs = node.stats(), node.range_stats()
        st["keys"] = node.keys()
    finally:
        node.close()
    return Outputs(*[np.concatenate([getattr(o, f) for o in outs]) for f in NC.FIELDS]), st, rs, p


def check_case(name, gpus, chunk_rows=0):
    got, st, rs, p = run_case(name, gpus, chunk_rows)
    assert_same(got, p.want)
    copies = len(p.routed.rows)
    assert sum(st["shard_rows"][:gpus]) == copies and rs.copies == copies and rs.rows == len(p.case.rows)
    assert st["keys"] == len(p.routed.keys)
    if gpus > 1:
        assert st["route_ms"] == 0 and st["merge_ms"] == 0      # no host work per row or per match
    return st


@pytest.mark.parametrize("gpus", [1, 2, 3, 4])
def test_three_overlapping_ranges_two_pushes(gpus):
    """DESIGN §3i's three ranges, state carried over two pushes, 'tiny' first held in the second; 'low' and 'tiny',
    which every event under 15 holds together, live on different shards at G = 2, 3 and 4"""
    c = NC.case("core")
    if gpus > 1:
        assert NC.shard(c.raw["low"], gpus) != NC.shard(c.raw["tiny"], gpus)
    st = check_case("core", gpus, chunk_rows=300)
    assert st["chunks"] == 3      # (of the second push: 700 rows)


@pytest.mark.parametrize("gpus", [1, 2, 3])
def test_written_range_order_beats_first_seen_order(gpus):
    c = NC.case("order")
    if gpus > 1:
        assert NC.shard(c.raw["tiny"], gpus) != NC.shard(c.raw["low"], gpus)
    check_case("order", gpus)


@pytest.mark.parametrize("gpus", [1, 2])
@pytest.mark.parametrize("n", NC.SLICE_ROWS)
def test_rows_per_slice_at_the_kernels_edges(n, gpus):
    """the second push is one chunk of n rows per GPU: under, at and over the 256-row step and the 2048-row block"""
    check_case(f"slice{n}x{gpus}", gpus)


def test_fewer_rows_than_gpus():
    check_case("few_rows", 4)


@pytest.mark.parametrize("gpus,chunk_rows", [(3, 5), (4, 700), (1, 5)])
def test_small_chunks(gpus, chunk_rows):
    """chunks with no copy at all, slices that send nothing to some shard and (G = 4, three labels) a shard that never
    gets a row"""
    st = check_case("chunks", gpus, chunk_rows)
    assert st["chunk_rows"] == chunk_rows
    if gpus == 4:
        assert 0 in st["shard_rows"][:4]


@pytest.mark.parametrize("gpus", [1, 4])
def test_32_ranges_all_held(gpus):
    """2049 rows x 32 copies: a full block of 65,536 copies and one row more; W = 32"""
    check_case("all32", gpus)


@pytest.mark.parametrize("gpus", [1, 4])
def test_32_ranges_one_held(gpus):
    check_case("one_of_32", gpus)


@pytest.mark.parametrize("gpus", [1, 2])
@pytest.mark.parametrize("name", ["unread_column", "null_condition", "one_stream", "shared_label", "value_and_ranges"])
def test_other_cases(name, gpus):
    check_case(name, gpus)


@pytest.mark.parametrize("no_fill", [False, True])
def test_one_gpu_host_fill_indexes_by_event(no_fill, monkeypatch):
    """closed form on one GPU: out->ts and the B-attribute columns come from the batch's trigger rows on the host; with
    SG_DEBUG_NODE_NO_FILL they come back from the GPU.  The same result, fewer bytes back."""
    if no_fill:
        monkeypatch.setenv("SG_DEBUG_NODE_NO_FILL", "1")
    else:
        monkeypatch.delenv("SG_DEBUG_NODE_NO_FILL", raising=False)
    got, st, _, p = run_case("core", 1, chunk_rows=300)
    assert_same(got, p.want)
    n2 = sum(1 for t in p.want.trigger if t >= p.case.base + 500)      # matches of the last push
    per_match = 8 + 4 + 4 + 4 + 1 + (8 + 4 + 4 + 1 + 1 if no_fill else 0)   # trigger key group p1 null (+ ts p2 v nulls)
    assert st["d2h_bytes"] == n2 * per_match


def test_sink_without_the_key_column():
    got, _, _, p = run_case("core", 2, chunk_rows=300, fields=("trigger", "ts", "group"))
    w = p.want
    assert_same(got, Outputs(w.trigger, w.ts, np.zeros(len(w), np.int32), w.group, w.vals, w.vnull))


def test_reset_keeps_the_ranges():
    p = NC.prepared("order")
    node = open_node(p, 2)
    try:
        n = len(p.case.rows)
        first = push(node, p, 0, n)
        node.reset()
        assert node.range_stats().copies == 0
        again = push(node, p, 0, n)
        assert node.range_stats().copies == len(p.routed.rows)
    finally:
        node.close()
    assert_same(first, p.want)
    assert_same(again, p.want)


# ------------------------------------------------------------------------------------------- refusals
def value_push_is_right(node, p: NC.Prepared):
    """the node still runs a plain value-partition push: rows of the core case keyed by the raw_key array alone (five
    keys, `volume % 5`), no range routing"""
    from siddhi_amd import _native as N
    from oracle import OracleEngine
    from siddhi_amd.runtime import Batch
    from parity_util import dense_first_seen
    b = p.batch
    n = 600
    key = (b.cols[2][:n] % 5).astype(np.int32)
    ob = Batch(n, 0, b.ts[:n], b.stream[:n], dense_first_seen(key), [x[:n] for x in b.cols],
               [None if x is None else x[:n] for x in b.nulls])
    eng = OracleEngine(p.ctx)
    eng.push(ob)
    want = eng.fetch()
    eng.close()
    assert len(want) > 0
    keep = []
    ts, raw = np.ascontiguousarray(ob.ts, np.int64), np.ascontiguousarray(key.astype(np.int64) * 977 + 13)
    st = np.ascontiguousarray(ob.stream, np.int32)
    cols = [np.ascontiguousarray(x) for x in ob.cols]
    nul = [None if x is None else np.ascontiguousarray(x, np.uint8) for x in ob.nulls]
    keep += [ts, raw, st] + cols + nul
    nb = N.make_node_batch(n, 0, ts.ctypes.data, st.ctypes.data, raw.ctypes.data, [x.ctypes.data for x in cols],
                           [0 if x is None else x.ctypes.data for x in nul], keep)
    sink = N.ColumnSink(p.nfa, 4 * n + 64, pinned=False)
    assert_same(node_outputs(p.nfa, sink, node.push(nb, sink.struct, sink.cap)), want)


def refused(node, desc, label_raw, code):
    from siddhi_amd._native import SgError
    with pytest.raises(SgError) as ei:
        node.set_ranges(desc, label_raw)
    assert ei.value.code == code, ei.value


@pytest.mark.parametrize("gpus", [1, 2])
def test_refusals_leave_a_working_node(gpus):
    from siddhi_amd import _native as N
    p = NC.prepared("core")
    good = N.build_range_desc(p.table)

    def changed(**kw):
        d = N.sg_range_desc.from_buffer_copy(good)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d
    # a condition deeper than the VM stack: 17 operands pushed before the first `and`
    deep_app = NC.C.parse(NC.app("volume>0 and (" * 16 + "price>1" + ")" * 16 + " as 'deep'"))
    part = deep_app.partitions[0]
    deep = N.build_range_desc(NC.L.lower_ranges(NC.L.make_context(deep_app, part.queries[0], part, {})))
    bad = [(changed(abi_version=3), SG_EINVAL), (changed(col_type=(1, NC.L.TYPE_CODE["LONG"])), SG_EINVAL),
           (changed(col_stream=(2, 1)), SG_EINVAL), (changed(n_cols=2), SG_EINVAL), (changed(n_ranges=0), SG_EINVAL),
           (deep, SG_EUNSUPPORTED)]
    for desc, code in bad:
        node = open_node(p, gpus, ranges=False)
        try:
            refused(node, desc, p.label_raw, code)
            value_push_is_right(node, p)
        finally:
            node.close()
    # after set_key_dict(1); and the host dictionary is refused once ranges are set
    node = open_node(p, gpus, ranges=False)
    try:
        node.set_key_dict(1)
        refused(node, good, p.label_raw, SG_EINVAL)
        value_push_is_right(node, p)
    finally:
        node.close()
    node = open_node(p, gpus)
    try:
        with pytest.raises(N.SgError) as ei:
            node.set_key_dict(1)
        assert ei.value.code == SG_EINVAL
        assert_same(push(node, p, 0, 500), _first_push(p))
        refused(node, good, p.label_raw, SG_EINVAL)      # after the first push
    finally:
        node.close()


def _first_push(p: NC.Prepared) -> Outputs:
    w = p.want
    m = w.trigger < p.case.base + 500
    return Outputs(*[getattr(w, f)[m] for f in NC.FIELDS])


ABSENT_APP = ("@app:playback define stream S (symbol string, price float, volume int); "
              "partition with (price>=50 as 'hi' or price<10 as 'lo' of S) begin @info(name='q') "
              "from every e1=S -> not S[volume==e1.volume] for 1 sec select e1.volume as v insert into M; end;")
PLAIN_APP = ("define stream S (symbol string, price float, volume int); @info(name='q') "
             "from every e1=S[price>10] -> e2=S[price>e1.price] within 1 sec "
             "select e1.price as p1, e2.price as p2, e2.volume as v insert into M;")


def test_queries_that_keep_the_host_route_are_refused():
    """playback timers (every shard needs every clock) and unpartitioned queries: SG_EUNSUPPORTED"""
    from siddhi_amd import _native as N
    p = NC.prepared("core")
    good = N.build_range_desc(p.table)
    a = NC.C.parse(ABSENT_APP)
    part = a.partitions[0]
    ctx = NC.L.make_context(a, part.queries[0], part, {})
    node = N.Node(N.build_desc(NC.L.lower(ctx)), n_gpus=2, devices=[0, 0], threads=4)
    try:
        refused(node, N.build_range_desc(NC.L.lower_ranges(ctx)), np.array([5, 6], np.int64), SG_EUNSUPPORTED)
    finally:
        node.close()
    a = NC.C.parse(PLAIN_APP)
    ctx = NC.L.make_context(a, a.queries[0], None, {})
    node = N.Node(N.build_desc(NC.L.lower(ctx)), n_gpus=1, devices=[0], threads=4)
    try:
        refused(node, good, p.label_raw, SG_EUNSUPPORTED)
    finally:
        node.close()


@pytest.mark.parametrize("gpus", [1, 2])
def test_base_index_beyond_the_internal_index(gpus):
    """three ranges: W = 4, so event indices stay below 2^61; the refused push leaves the node usable"""
    from siddhi_amd._native import SgError
    p = NC.prepared("core")
    node = open_node(p, gpus)
    try:
        with pytest.raises(SgError) as ei:
            push(node, p, 0, 500, base=(1 << 61) - 100)
        assert ei.value.code == SG_EINVAL
        assert_same(push(node, p, 0, 500), _first_push(p))
    finally:
        node.close()
