"""The aggregation stage (csrc/agg.hip: k_agg_groups, the slot sort, k_agg_tiles / k_agg_carry / k_agg_scan,
k_agg_serial, k_agg_writeback) on the GPU against the oracle's base records folded by agg_ref.py, bit for bit (nulls
agree, any NaN equals any NaN of its width): every aggregator and argument type, the group shapes, run lengths around
the scan's block (256 records, one tile), the group table's growth, the serial fallback of avg over LONG, the routes
that feed the selector, snapshot / restore, egress, the entry point's refusals and the host API."""
import ctypes as ct
import os

import numpy as np
import pytest

import agg_cases as A
import agg_ref as R
from parity_util import context
from siddhi_amd import lowering as L

pytestmark = pytest.mark.gpu

BLOCK = 256      # AGG_BLOCK of agg.hip: threads per block = records per scan tile


def run_gpu(case, app=None, **kw):
    """(per push Outputs, per push kernel names) of the HIP engine over the case's aggregate app"""
    from siddhi_amd._native import GpuEngine
    log = []

    class Witness(GpuEngine):
        def __init__(self, ctx):
            super().__init__(ctx, **{**case.engine_kw, **kw})

        def push(self, b):
            super().push(b)
            log.append([name for name, _ in self.handle.timing().kernels()])

    return A.run_pushes(Witness, app or case.agg_app(), case.batches()), log


@pytest.mark.parametrize("case", A.ALL, ids=str)
def test_agg_values(case):
    got, log = run_gpu(case)
    A.check(case, got, "gpu ")
    names = [n for p in log for n in p]
    assert "agg_groups" in names and "agg_writeback" in names, log


def test_avg_long_fallback_is_reached():
    """partial sums cross 2^53: the runs are redone by k_agg_serial (kernel mark), and only then"""
    _, log = run_gpu(A.AVG53)
    assert any("agg_serial_avg53" in p for p in log), log
    _, log = run_gpu(A.AVG_EXACT)
    assert not any("agg_serial_avg53" in p or "agg_serial" in p for p in log), log


# ---- run shapes around the scan's block: the group column decides the runs --------------------------------------
def _shape_case(name, group_of_match, **kw):
    """Rows alternate p = 30, 40: every odd row completes exactly the e1 of the row before it (the 40s wait for a higher
    p that never comes), so match m is (row 2m, row 2m + 1), in row order.  The e2 row carries the group:
    gl = group_of_match(m).  The runs of the sorted order then have exactly the lengths the shape asks for."""
    c = A.Case(name, [("count", None, "INT"), ("sum", "e2.lv", "LONG"), ("max", "e2.fv", "FLOAT"),
                      ("min", "e2.dv", "DOUBLE"), ("avg", "e2.iv", "INT")], [("e2.gl", "LONG")], part=False,
               null_frac=0.0, **kw)
    base_batches = c.batches

    def batches():
        out = base_batches()
        lo = 0
        for b in out:
            rows = np.arange(lo, lo + b.n, dtype=np.int64)
            b.cols[A.COLS.index("p")] = np.where(rows % 2 == 0, 30, 40).astype(np.int32)
            b.cols[A.COLS.index("gl")] = np.asarray(group_of_match(rows // 2)).astype(np.int64)
            b.nulls[A.COLS.index("gl")] = None
            lo += b.n
        return out
    c.batches = batches
    return c


EDGE_RUNS = [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 1, 3 * BLOCK + 7]     # the last one spans more than three tiles


def _runs_of(lengths):
    """match -> group so that group g owns exactly lengths[g] matches, interleaved (the sort gathers them)"""
    owner = np.repeat(np.arange(len(lengths)), lengths)
    np.random.default_rng(5).shuffle(owner)
    return lambda m: owner[np.minimum(m, len(owner) - 1)]


SHAPES = [
    _shape_case("shape-one-group", lambda m: np.zeros(len(m)), n=1200),
    _shape_case("shape-own-groups", lambda m: m, n=1200),
    _shape_case("shape-block-edges", _runs_of(EDGE_RUNS), n=2 * sum(EDGE_RUNS)),
    _shape_case("shape-block-edges-3push", _runs_of(EDGE_RUNS), n=2 * sum(EDGE_RUNS), cuts=[2, 1500, 1502]),
    _shape_case("shape-empty-push", lambda m: m % 3, n=1200, cuts=[700, 700, 1100]),
]


@pytest.mark.parametrize("case", SHAPES, ids=str)
def test_run_shapes(case):
    base = A.base_outputs(case)
    assert sum(len(o) for o in base) == case.n // 2      # one match per row pair
    got, _ = run_gpu(case)
    A.check(case, got, "gpu ")
    if case.name == "shape-block-edges":      # the runs of the sorted order are the lengths asked for
        lens = np.unique(base[0].vals[:, 0], return_counts=True)[1]
        assert sorted(lens.tolist()) == sorted(EDGE_RUNS)


# ---- the scan's second level: k_agg_carry is one block whose 256 threads each fold a chunk of ceil(tiles / 256) tiles,
# so up to 256 tiles (65,536 matches) a chunk is one tile and above that a thread folds several, scans the chunk folds
# over the block and walks its chunk again.  One match either side of that size, and a push of 200,001 matches (782
# tiles, chunks of 4 tiles = 1,024 records) with runs that span several threads' chunks and runs that start inside one.
CARRY = BLOCK * 256


def _filled(head, total, unit=777):
    """run lengths: `head`, then runs of `unit`, then the rest, `total` matches in all"""
    rest = total - sum(head)
    return head + [unit] * (rest // unit) + ([rest % unit] if rest % unit else [])


MIXED = [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 5000, 333]
BIG = 200_001
BIG_RUNS = _filled([1, 1023, 1024, 1025, 5000, 70_001, 333, 4 * 1024 + 1], BIG)
# (rows 100 ms apart: few e1 wait inside `within 1 sec`, which keeps the oracle's share of a case small)
CARRY_CASES = [
    _shape_case("carry-65535-runs", _runs_of(_filled(MIXED, CARRY - 1)), n=2 * (CARRY - 1), ts_step=100),
    _shape_case("carry-65536-runs", _runs_of(_filled(MIXED, CARRY)), n=2 * CARRY, ts_step=100),
    _shape_case("carry-65537-runs", _runs_of(_filled(MIXED, CARRY + 1)), n=2 * (CARRY + 1), ts_step=100),
    _shape_case("carry-65537-one-group", lambda m: np.zeros(len(m)), n=2 * (CARRY + 1), ts_step=100),
    _shape_case("carry-65537-own-groups", lambda m: m, n=2 * (CARRY + 1), ts_step=100),
    _shape_case("carry-200001-runs", _runs_of(BIG_RUNS), n=2 * BIG, ts_step=100),
    _shape_case("carry-200001-one-group-3push", lambda m: np.zeros(len(m)), n=2 * BIG, ts_step=100, cuts=[2, 2 * 70_000]),
]


@pytest.mark.parametrize("case", CARRY_CASES, ids=str)
def test_carry_chunks(case):
    base = A.base_outputs(case)
    assert sum(len(o) for o in base) == case.n // 2
    got, log = run_gpu(case)
    A.check(case, got, "gpu ")
    assert any("agg_carry" in p for p in log), log
    if case.name == "carry-200001-runs":
        lens = np.unique(base[0].vals[:, 0], return_counts=True)[1]
        assert sorted(lens.tolist()) == sorted(BIG_RUNS)


# ---- table ------------------------------------------------------------------------------------------------------
def test_table_grows_in_the_middle_of_a_push():
    """more groups than the table's first 512 slots, most of them first seen inside one push; a group first seen in the
    last push"""
    case = _shape_case("table-growth", lambda m: np.where(m < 1350, m % 1200, 5000 + m), n=3000, cuts=[300, 2600])
    got, _ = run_gpu(case)
    A.check(case, got, "gpu ")


def test_direct_next_to_hashed():
    """the same stream grouped by the partition attribute (hashed) and not grouped (direct, slot = partition key)"""
    aggs = [("count", None, "INT"), ("sum", "e2.iv", "INT"), ("max", "e2.dv", "DOUBLE")]
    direct = A.Case("direct", aggs, cuts=A._cuts3(1500), keys=40)
    hashed = A.Case("hashed", aggs, [("e1.symbol", "STRING")], cuts=A._cuts3(1500), keys=40)
    gd, _ = run_gpu(direct)
    gh, _ = run_gpu(hashed)
    A.check(direct, gd, "gpu ")
    A.check(hashed, gh, "gpu ")
    for d, h in zip(gd, gh):
        assert np.array_equal(d.vals, h.vals[:, 1:]) and np.array_equal(d.vnull, h.vnull[:, 1:])


# ---- routes -----------------------------------------------------------------------------------------------------
SMALL = [("count", None, "INT"), ("sum", "e2.lv", "LONG"), ("avg", "e2.dv", "DOUBLE"), ("max", "e2.fv", "FLOAT")]
ONCE = "from e1=S[p>20] -> e2=S[p > e1.p]"
# (e3 is null where e4 completed the logical state: null arguments)
LANE = [("count", None, "INT"), ("sum", "e3.lv", "LONG"), ("avg", "e4.dv", "DOUBLE"), ("max", "e2[last].fv", "FLOAT")]
ROUTES = {
    "tiled": (A.Case("route-tiled", SMALL, [("e1.gi", "INT")], cuts=A._cuts3(1500)),
              (("walk_count",), ("nge_search", "nfa_keys", "nfa_units"))),
    "wide": (A.Case("route-wide", SMALL[:2], [("e1.gi", "INT")], n=140_000, keys=70_000, cuts=[70_000]),
             (("walk_count", "group_walk"), ("nge_search", "nfa_keys", "nfa_units"))),
    "search": (A.Case("route-search", SMALL, [("e1.gi", "INT")], part=False, cuts=A._cuts3(1500)),
               (("nge_search",), ("walk_count", "nfa_keys", "nfa_units"))),
    "lanes": (A.Case("route-lanes", SMALL, [("e1.gi", "INT")], part=False, cuts=A._cuts3(1500),
                     engine_kw={"force_general": True}),
              (("partial_lanes",), ("walk_count", "nge_search", "nfa_keys", "nfa_units"))),
    "machine": (A.Case("route-machine", SMALL, [("e1.gi", "INT")], cuts=A._cuts3(1500),
                       engine_kw={"force_general": True, "partial_lanes": -1}),
                (("nfa_keys", "nfa_units"), ("walk_count", "nge_search", "partial_lanes"))),
    # timer-emitted matches: an e1 whose lv no row repeats for 5 sec (about half of them are killed)
    "absent": (A.Case("route-absent", [("count", None, "INT"), ("sum", "e1.iv", "INT"), ("avg", "e1.dv", "DOUBLE"),
                                       ("max", "e1.fv", "FLOAT")], [("e1.gi", "INT")], part=False,
                      pattern="from every e1=S -> not S[lv==e1.lv] for 5 sec", app_head="@app:playback ", ts_step=20,
                      pools={"lv": list(range(400))}, null_frac=0.0, cuts=A._cuts3(1500)),
               (("abs_roles",), ("abs_sequential", "nfa_keys", "nfa_units"))),
    "partial_lanes": (A.Case("route-partial-lanes", LANE, [("e1.gi", "INT")], n=6000, cuts=A._cuts3(6000),
                             pattern="from every e1=S[p>40] -> e2=S[p>e1.p]<2:5> -> e3=S[p<e1.p] and e4=S[iv<e1.iv] "
                                     "within 1 sec"),
                      (("partial_lanes",), ("nfa_keys", "nfa_units"))),
    "sequence_lanes": (A.Case("route-sequence-lanes", LANE, [("e1.gi", "INT")], n=6000, cuts=A._cuts3(6000),
                              pattern="from every e1=S[p>40], e2=S[p>e1.p]<1:5>, e3=S[p<e1.p] or e4=S[iv<e1.iv]"),
                       (("sequence_lanes",), ("nfa_keys",))),
    "once": (A.Case("route-once", SMALL, [("e1.gi", "INT")], pattern=ONCE, keys=400, n=3000, cuts=[1000, 2000]),
             (("once_match",), ("nfa_keys", "nfa_units"))),
}


@pytest.mark.parametrize("route", list(ROUTES), ids=str)
def test_routes(route):
    case, (some, none) = ROUTES[route]
    got, log = run_gpu(case)
    assert sum(len(g) for g in got) >= 200
    A.check(case, got, "gpu ")
    names = [n for p in log for n in p]
    assert any(n in names for n in some) and not any(n in names for n in none), (route, log)


# ---- snapshot / restore -----------------------------------------------------------------------------------------
SNAP = A.Case("snapshot", A.ALL5, [("e1.gs", "STRING"), ("e2.gf", "FLOAT")], cuts=A._cuts3(1500))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "plain_snapshot.bin")
PLAIN_APP = A.Case("plain", []).base_app()


def _engine(app, **kw):
    from siddhi_amd._native import GpuEngine
    return GpuEngine(context(app), **kw)


def test_snapshot_at_every_cut():
    batches = SNAP.batches()
    whole, _ = run_gpu(SNAP)
    blobs = []
    for cut in range(len(batches) + 1):
        a = _engine(SNAP.agg_app())
        for b in batches[:cut]:
            a.push(b)
            a.fetch()
        blob = a.snapshot()
        blobs.append(blob)
        a.close()
        b2 = _engine(SNAP.agg_app())
        b2.restore(blob)
        rest = []
        for b in batches[cut:]:
            b2.push(b)
            rest.append(b2.fetch())
        assert b2.snapshot() == _final_blob(batches), f"cut {cut}: the restored handle ends in another state"
        b2.close()
        for g, w in zip(rest, whole[cut:]):
            assert np.array_equal(g.vals, w.vals) and np.array_equal(g.vnull, w.vnull), f"cut {cut}"
            assert np.array_equal(g.trigger, w.trigger)
    A.check(SNAP, whole, "gpu ")


_FINAL = {}


def _final_blob(batches):
    """two handles fed the same pushes give identical blob bytes: the first one's final blob is kept, every later
    handle's is compared with it"""
    e = _engine(SNAP.agg_app())
    for b in batches:
        e.push(b)
        e.fetch()
    blob = e.snapshot()
    e.close()
    assert _FINAL.setdefault("blob", blob) == blob
    return blob


def test_blob_of_other_aggregates_is_refused():
    from siddhi_amd._native import SgError
    a = _engine(SNAP.agg_app())
    for b in SNAP.batches()[:2]:
        a.push(b)
        a.fetch()
    blob = a.snapshot()
    a.close()
    other = _engine(SNAP.agg_app().replace("max(e2.fv)", "min(e2.fv)"))
    with pytest.raises(SgError, match="another query"):
        other.restore(blob)
    other.close()


def test_plain_blob_is_the_one_from_before_aggregates():
    """a query without aggregates: the blob bytes of the commit before sg_set_aggregates existed (tests/golden)"""
    e = _engine(PLAIN_APP)
    for b in A.Case("plain", []).batches():
        e.push(b)
        e.fetch()
    blob = e.snapshot()
    e.close()
    with open(GOLDEN, "rb") as f:
        assert blob == f.read()


# ---- egress -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["poll_columns", "push_deliver"])
def test_egress_delivers_result_types(how):
    from siddhi_amd._native import ColumnSink, GpuEngine, column_dtypes
    case = A.Case("egress", A.ALL5, [("e1.gs", "STRING")])
    eng = GpuEngine(context(case.agg_app()))
    assert column_dtypes(eng.nfa) == [np.int32, np.int64, np.int64, np.float64, np.float32, np.float64]
    sink = ColumnSink(eng.nfa, 4096)
    keep = []
    (b,) = case.batches()
    if how == "poll_columns":
        eng.push(b)
        n = eng.handle.poll_columns(sink.struct, 4096)
    else:
        n = eng.handle.push_deliver(eng._host_batch(b, keep), sink.struct, 4096)
    eng.close()
    _, rows = A.expected(case)
    assert n == len(rows[0]) > 200
    rtypes = ["STRING"] + [R.result_type(nm, t) for nm, _, t in case.aggs]
    for j, (_, vals) in enumerate(rows[0]):
        for k, want in enumerate(vals):
            col, nul = sink.cols[1 + k], sink.nulls[1 + k]
            assert bool(nul[j]) == (want is None)
            if want is not None:
                t = rtypes[1 + k]
                gb = col[j:j + 1].view({"FLOAT": np.uint32, "DOUBLE": np.int64}.get(t, col.dtype))[0]
                assert R.same_value(gb, want, t), (j, k, col[j], want)


def test_ingress_chunks_are_consecutive_pushes():
    """sg_push cuts a host batch into chunks (ingress_rows): the stage runs per chunk in order on the carried group state"""
    case = A.Case("chunks", A.ALL5, [("e1.gs", "STRING"), ("e2.gf", "FLOAT")])
    got, log = run_gpu(case, ingress_rows=97)
    A.check(case, got, "gpu ")


# ---- entry-point misuse -----------------------------------------------------------------------------------------
def test_set_aggregates_misuse():
    from siddhi_amd import _native as N
    case = A.Case("misuse", A.ALL5, [("e1.gs", "STRING")])
    nfa = L.lower(context(case.agg_app()))
    (b,) = case.batches()

    def fresh():
        return N.Handle(N.build_desc(nfa))

    def rc(h, a):
        return h.lib.sg_set_aggregates(h.h, ct.byref(a))

    good = N.build_agg_desc(nfa)
    for field, value, code in (("abi_version", 99, -1), ("n_out", 3, -1), ("n_out", 0, -1), ("n_group", 5, -1),
                               ("n_group", -1, -1), ("code_len", 65, -1)):
        h = fresh()
        bad = N.build_agg_desc(nfa)
        setattr(bad, field, value)
        assert rc(h, bad) == code, field
        assert rc(h, good) == 0       # the refused call left a working handle
        h.close()
    h = fresh()
    bad = N.build_agg_desc(nfa)
    bad.kind[1] = 9
    assert rc(h, bad) == -1
    bad = N.build_agg_desc(nfa)
    bad.kind[0], bad.kind[1], bad.kind[2], bad.kind[3], bad.kind[4], bad.kind[5] = 0, 0, 0, 0, 0, 0
    assert rc(h, bad) == -1           # no aggregate column
    bad = N.build_agg_desc(nfa)
    bad.code[0], bad.group_off[0], bad.group_len[0], bad.code_len = L.OP_VAR, 0, 1, 1
    assert rc(h, bad) == -1           # a group-by program that ends inside its VAR instruction
    assert b"inside an instruction" in h.lib.sg_last_error(h.h)
    h.close()
    h = fresh()
    assert rc(h, good) == 0
    assert rc(h, good) == -1 and b"already" in h.lib.sg_last_error(h.h)      # twice
    h.close()
    eng = N.GpuEngine(context(case.base_app()))       # a plain handle: after its first push
    eng.push(b)
    eng.fetch()
    plain_nfa = eng.nfa
    a = N.sg_agg_desc()
    a.abi_version, a.n_out = N.SG_AGG_ABI_VERSION, len(plain_nfa.out_progs)
    assert rc(eng.handle, a) == -1 and b"after" in eng.handle.lib.sg_last_error(eng.handle.h)
    eng.push(b)                       # still a working handle
    assert len(eng.fetch()) > 0
    eng.close()


def test_deep_group_program_is_unsupported():
    from siddhi_amd import _native as N
    case = A.Case("deep", [("count", None, "INT")], [("e1.gi", "INT")])
    nfa = L.lower(context(case.agg_app()))
    a = N.build_agg_desc(nfa)
    # 17 operands on the stack before the first MATH pops (constants: 3 words each fit the 64-word code array)
    prog = [L.OP_CONST, 1, 1] * 17 + [L.OP_MATH, 0, 1] * 4
    assert len(prog) <= N.SG_AGG_MAX_CODE
    for k, w in enumerate(prog):
        a.code[k] = w
    a.group_off[0], a.group_len[0], a.code_len = 0, len(prog), len(prog)
    h = N.Handle(N.build_desc(nfa))
    assert h.lib.sg_set_aggregates(h.h, ct.byref(a)) == N.SG_EUNSUPPORTED
    assert b"deeper than the VM stack" in h.lib.sg_last_error(h.h)
    h.close()


# ---- host API ---------------------------------------------------------------------------------------------------
ISSUE_APP = """define stream S (symbol string, price float, volume int);
partition with (symbol of S) begin @info(name='q')
from every e1=S[price>20] -> e2=S[price > e1.price] within 1 sec
select e1.symbol as s, count() as n, sum(e2.volume) as vol, avg(e2.price - e1.price) as gain, max(e2.price) as hi
group by e1.symbol having n > 3 insert into M; end;"""


def test_host_api_delivers_the_rows():
    from siddhi_amd.runtime import QueryCallback, SiddhiManager
    rng = np.random.default_rng(3)
    rows = [(1000 + i, [f"K{int(rng.integers(0, 3))}", float(np.float32(15 + 0.5 * int(rng.integers(0, 60)))),
                        int(rng.integers(1, 100))]) for i in range(400)]
    # the rules, once more, on this stream: every e1 with price > 20 waits for the first later row of its symbol with a
    # higher price (within 1 sec: every row is); rows delivered in order of the completing row, then of e1
    want, state, pending = [], {}, {}
    for ts, (sym, price, vol) in rows:
        done = [e1 for e1 in pending.get(sym, []) if price > e1]
        pending[sym] = [e1 for e1 in pending.get(sym, []) if not price > e1]
        for e1 in done:
            st = state.setdefault(sym, {"n": 0, "vol": 0, "gain": 0.0, "hi": None})
            st["n"] += 1
            st["vol"] += vol
            st["gain"] += float(np.float32(np.float32(price) - np.float32(e1)))
            st["hi"] = price if st["hi"] is None or st["hi"] < price else st["hi"]
            if st["n"] > 3:
                want.append([sym, st["n"], st["vol"], st["gain"] / st["n"], st["hi"]])
        if price > 20:
            pending.setdefault(sym, []).append(price)
    got = []

    class CB(QueryCallback):
        def receive(self, timestamp, inEvents, removeEvents):
            got.extend(e.data for e in inEvents)

    rt = SiddhiManager().createSiddhiAppRuntime(ISSUE_APP)
    rt.addCallback("q", CB())
    ih = rt.getInputHandler("S")
    rt.start()
    for ts, data in rows:
        ih.send(ts, data)
    rt.shutdown()
    assert len(want) > 50
    assert got == want
