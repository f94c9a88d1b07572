"""The cases of test_snapshot_cases.py (CPU guard) and test_snapshot_cuts.py (GPU): the smallest streams that still carry
state over a cut, for every serialiser behind sg_snapshot / sg_restore, each cut at a dozen or more places.

A case is a query text, engine options and one stream of rows; nothing here restates a pattern or a row generator:
the every-next and once cases are value_cases.CLOSED cases (edge pools, 3 % nulls), the lane cases are the shapes and
streams of test_partial_lanes.py, the absence cases those of test_absent_closed_form.py, the growth stream that of
test_capacity.py.  A heartbeat (sg_advance_time) is a row of stream -1 in the stream: the oracle takes it as a clock-only
row, the drivers send it through Handle.advance_time.

Cuts are placed from the oracle's output over the uninterrupted stream (place_cuts): a cut that no state has to cross
proves nothing, so every cut is straddled by a match whose e1 row lies before it and whose trigger row at or after it
(every query here selects e1's row number first).  The drivers at the end hop the state between handles in four ways."""
import zlib
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

import value_cases as V
from oracle import OracleEngine
from parity_util import context, dense_first_seen
from siddhi_amd import lowering as L
from siddhi_amd import synth
from siddhi_amd.runtime import Batch, Outputs
from test_absent_closed_form import EDGE_APPS, W, _edge_batch, c4_batch
from test_capacity import Q as GROWTH_Q
from test_capacity import skewed
from test_partial_lanes import (HEAD, SEQ_SHAPES, SHAPES, UNPART, UNPART_SEQ, _going_back, _long_seq, _rising_runs,
                                small_batch)

DAY = 86_400_000
STEPS = (1, 2, 3, 5, 8, 13, 21, 34)
FIELDS = ("trigger", "ts", "key", "group", "vals", "vnull")


@dataclass
class SnapCase:
    name: str
    family: str                   # every / once / absent / machine / lanes / seq: the serialiser the state travels in
    app: str
    make: Callable[[], Batch]     # the whole stream
    engine: dict = field(default_factory=dict)       # GpuEngine keywords
    floor: int = 0                # oracle matches over the whole stream, at least
    source: Optional[V.Case] = None                  # the value_cases case an every / once case is
    shape: str = ""               # the name in SHAPES / SEQ_SHAPES of a lane or machine case
    must_cut: tuple = ()          # cuts the case is about (a heartbeat just before, a late row just after)
    near: tuple = ()              # rows at or shortly after which a cut is wanted
    id_col: Optional[int] = None  # absence queries: the column of the compared id (the decoy doubles the ids)
    sparse_nulls: bool = False    # a piece without a null in a column is pushed without that column's null flags
    sequential: bool = False      # absence closed form: some push runs the sequential pass (a late row)
    seq_small: Optional[bool] = None                 # sequence lanes: the state layout the shape takes

    def __str__(self):
        return self.name


# ---------------------------------------------------------------------------------------------- streams
def _from(b: Batch, rows) -> Batch:
    return Batch(len(rows), 0, b.ts[rows], b.stream[rows], b.key[rows], [np.ascontiguousarray(c[rows]) for c in b.cols],
                 [None if x is None else np.ascontiguousarray(x[rows]) for x in b.nulls])


def _shape_stream(name, n=600, keys=5):
    return small_batch(n, keys, 100, 4, seed=sum(name.encode()) + 1)


def _with_nulls(name):
    """null flags on v in some pushes only (rows 150 .. 399), as test_nulls_stay_on_partial_lanes has them in push 2"""
    b = _shape_stream(name)
    nul = np.zeros(b.n, np.uint8)
    nul[150:400] = np.random.default_rng(3).random(250) < 0.05
    b.nulls[2] = nul
    return b


def _back(rows=600):
    """_going_back scaled down: its first `rows` rows and the first `rows` of its second half (the same keys again),
    moved so that they start 400 ms before the first part's end, as the whole second half does there"""
    g = _going_back(None, back=400)
    b = _from(g, np.concatenate([np.arange(rows), 10_000 + np.arange(rows)]))
    b.ts[rows:] -= g.ts[9_999] - g.ts[rows - 1]
    assert b.ts[rows] == b.ts[rows - 1] + 1 - 400
    b.cols[0] = np.arange(b.n, dtype=np.int64)       # id = row number
    return b


EDGE_N = 2000


def _edge(name, n=EDGE_N):
    """_edge_batch(gap_max=400, null_frac=0.1, ids=200) and a closing clock-only row that fires what is left"""
    rng = np.random.default_rng(zlib.crc32(f"snapshot/{name}".encode()))
    _, b = _edge_batch(EDGE_APPS[name], rng, n, 200, 400, 0.1)
    return b


def _closed(b: Batch, after: int) -> Batch:
    """b and one more row, `after` ms later, on a stream no state reads: clock only (stream -1, a heartbeat)"""
    return Batch(b.n + 1, 0, np.append(b.ts, b.ts[-1] + after), np.append(b.stream, np.int32(-1)).astype(np.int32),
                 np.zeros(b.n + 1, np.int32), [np.append(c, 0).astype(c.dtype) for c in b.cols],
                 [None if x is None else np.append(x, 0).astype(np.uint8) for x in b.nulls])


def _edge_time_back():
    """`flip` (for 1 sec): from row 800 on every row lies 700 ms earlier, so row 800 arrives behind the clock, the
    closed form hands over to its sequential pass (as->seq) and lastScheduledTime (lst) is ahead of the rows"""
    b = _edge("flip")
    b.ts[800:] -= 700
    assert b.ts[800] < b.ts[799]
    return _closed(b, 1001)


def _stretched_c4(n, ids):
    """c4_batch (its closing Tick row included) at 4 ms per row: timers (5 s) fire inside the stream too"""
    b = c4_batch(n, ids)
    b.ts = b.ts[0] + 4 * (b.ts - b.ts[0])
    return b


def _c4_late_row():
    """Row 1,000 is a Tick row 20 s ahead: the clock runs on, every timer of the rows before fires and the scheduler's
    FIFO is empty (it fires from its head only, so a timer that is not due would hide the ones behind it).  The rows
    after it are back on the old time line at 8 ms per row, far more than `for` = 5 s behind the clock, before and after
    the cut at 1,200.  A row behind the clock does not notify the scheduler (TimestampGeneratorImpl.setCurrentTimestamp),
    so nothing fires until the closing row; an engine whose clock fell back to the rows' own time would see the late
    rows move it and fire their timers from row 1,626 on."""
    b = _stretched_c4(2000, 500)
    b.stream[1000] = 1
    b.ts[1000] += 20_000
    b.ts[1001:2000] = b.ts[999] + 8 * np.arange(1, 1000)
    clock = b.ts[1000]
    b.ts[-1] = clock + W + 1
    assert clock - b.ts[1999] > W and b.ts[1001] + W < b.ts[1999] and b.stream[-1] == 1
    return b


HB_ROW = 600


def _c4_heartbeat():
    """a heartbeat (a row of stream -1) at row 600, 4 s after the row before it: the timers of the first 350 rows fire
    at it, the younger partials stay pending across the cut that follows.  The rows after it go on where the stream
    was, behind the clock for 1,000 rows (they move no clock and notify no scheduler), then ahead of it again."""
    b = _stretched_c4(2000, 500)
    hb = int(b.ts[HB_ROW - 1]) + 4000
    assert b.ts[HB_ROW] < hb < b.ts[1999] and hb > b.ts[0] + W
    ins = lambda a, v: np.insert(a, HB_ROW, v).astype(a.dtype)   # noqa: E731
    return Batch(b.n + 1, 0, ins(b.ts, hb), ins(b.stream, -1), np.zeros(b.n + 1, np.int32),
                 [ins(c, 0) for c in b.cols], [None] * 3)


# ---------------------------------------------------------------------------------------------- the cases
EVERY_NAMES = (
    [f"carry-{t}-{op}-{m}" for t in V.TYPES for op, m in ((">", "stack"), ("<=", "list"))] +
    ["search-INT->", "search-DOUBLE-<=", "flat_walker-LONG->", "flat_walker-FLOAT-<=", "sorted-INT-<=", "sorted-LONG->",
     "redo-FLOAT->-stack", "redo-DOUBLE-<=-list", "wide-LONG->-pushes", "wide-DOUBLE-<=-pushes", "wide-INT->-pushes",
     "time_back-FLOAT->", "time_back-DOUBLE-<=", "two_streams-INT->", "two_streams-LONG-<=", "two_streams-FLOAT->"])
ONCE_NAMES = [f"once-{t}->-split" for t in V.TYPES]

# the new small streams: half of what the oracle delivers over the whole stream at the committed seeds (the every-next
# and once cases keep the floors of value_cases.py)
FLOORS = {"absent-filters": 916, "absent-flip": 978, "absent-int_attr": 942, "absent-time_back": 978,
          "absent-c4-heartbeat": 318, "machine-c3c": 117, "machine-seq_c3b": 11, "machine-c4": 244,
          "machine-c4-late_row": 427, "machine-c4-heartbeat": 318, "lanes-and": 124, "lanes-and_next": 38,
          "lanes-c3c": 117, "lanes-count13": 191, "lanes-count22": 189, "lanes-count_or": 224,
          "lanes-filter_cross": 120, "lanes-next": 138, "lanes-next3": 150, "lanes-or": 150, "lanes-unpart": 133,
          "lanes-next-nulls": 136, "lanes-count13-nulls": 190, "lanes-count13-time_back": 289,
          "lanes-c3c-time_back": 109, "lanes-next3-lateness0": 150, "lanes-next3-time_back-lateness400": 211,
          "seq-seq_and": 16, "seq-seq_c3b": 11, "seq-seq_count": 56, "seq-seq_cross": 174, "seq-seq_last_ref": 22,
          "seq-seq_next": 192, "seq-seq_or_next": 186, "machine-unpart_seq": 19, "seq-long5": 194}


def _value_case(name, family):
    c = V.BY_NAME[name]
    return SnapCase(name, family, c.app, lambda: V.batch(c), engine=dict(c.engine), floor=c.floor, source=c)


def _lane(name, shape, make, q=None, **kw):
    engine = dict(force_general=True, **kw.pop("engine", {}))
    return SnapCase(name, "lanes", HEAD + (SHAPES[shape] if q is None else q), make, engine=engine, shape=shape, **kw)


def _seq(name, shape, make, q=None, small=True):
    """Every shape of SEQ_SHAPES has at most 4 states, 6 count-chain entries and 3 elements (a logical
    pair is one element), so seq.h sg_seq_small gives each of them the 124-byte SeqStateT<SqSmall>: seq_c3b is the
    largest with 4 states, a chain of 5 and pool 4.  The 236-byte SeqState is taken by test_partial_lanes._long_seq(5):
    5 elements make a pool of 6 partials (the route's bound, PQ_MAX_P)."""
    return SnapCase(name, "seq", q if q is not None else HEAD + SEQ_SHAPES[shape], make, shape=shape, seq_small=small)


def cases() -> List[SnapCase]:
    out = [_value_case(n, "every") for n in EVERY_NAMES] + [_value_case(n, "once") for n in ONCE_NAMES]
    # absence closed form
    for name in sorted(EDGE_APPS):
        out.append(SnapCase(f"absent-{name}", "absent", EDGE_APPS[name], lambda name=name: _closed(_edge(name), 3001),
                            id_col=0, must_cut=(EDGE_N,)))
    out.append(SnapCase("absent-time_back", "absent", EDGE_APPS["flip"], _edge_time_back, id_col=0, near=(801,),
                        must_cut=(EDGE_N,), sequential=True))
    out.append(SnapCase("absent-c4-heartbeat", "absent", synth.QUERIES["C4"], _c4_heartbeat, id_col=0,
                        must_cut=(HB_ROW, HB_ROW + 1)))
    # the per-key machine (arena route)
    M = dict(force_general=True, partial_lanes=-1)
    out.append(SnapCase("machine-c3c", "machine", HEAD + SHAPES["c3c"], lambda: _shape_stream("c3c"), engine=M,
                        shape="c3c"))
    out.append(SnapCase("machine-seq_c3b", "machine", HEAD + SEQ_SHAPES["seq_c3b"],
                        lambda: _rising_seq("seq_c3b"), engine=M, shape="seq_c3b"))
    G = dict(force_general=True, pool=16384)
    out.append(SnapCase("machine-c4", "machine", synth.QUERIES["C4"], lambda: c4_batch(2000, 500), engine=G, id_col=0))
    out.append(SnapCase("machine-c4-late_row", "machine", synth.QUERIES["C4"], _c4_late_row, engine=G, id_col=0,
                        must_cut=(1200,)))
    out.append(SnapCase("machine-c4-heartbeat", "machine", synth.QUERIES["C4"], _c4_heartbeat, engine=G, id_col=0,
                        must_cut=(HB_ROW, HB_ROW + 1)))
    # partial lanes
    for name in sorted(SHAPES):
        out.append(_lane(f"lanes-{name}", name, lambda name=name: _shape_stream(name)))
    out.append(_lane("lanes-unpart", "", lambda: small_batch(600, 1, 100, 2, seed=3), q=UNPART))
    for name in ("next", "count13"):
        out.append(_lane(f"lanes-{name}-nulls", name, lambda name=name: _with_nulls(name), sparse_nulls=True))
    for name in ("count13", "c3c"):
        out.append(_lane(f"lanes-{name}-time_back", name, _back))
    # bounded lateness.  A bound of 0 promises that no row arrives behind the largest timestamp so far, which the stream
    # going back 400 ms breaks (the engine then drops partials the reference keeps, by the option's design): next3 runs
    # with the bound 0 on its monotone stream, and with the bound 400 ms, which that stream keeps, on the one going back
    out.append(_lane("lanes-next3-lateness0", "next3", lambda: _shape_stream("next3"),
                     engine=dict(max_lateness_ms=0)))
    out.append(_lane("lanes-next3-time_back-lateness400", "next3", _back,
                     engine=dict(max_lateness_ms=400)))
    # sequence lanes
    for name in sorted(SEQ_SHAPES):
        out.append(_seq(f"seq-{name}", name, (lambda name=name: _rising_seq(name)) if name in RISING else
                        (lambda name=name: _shape_stream(name))))
    # UNPART_SEQ is no sequence-lane query: without a partition the start state keeps withinEvery (lowering.py), which
    # seq.h sg_seq_rule refuses, so its state travels in the per-key machine's arena -- with no option forcing it there
    out.append(SnapCase("machine-unpart_seq", "machine", HEAD + UNPART_SEQ,
                        lambda: small_batch(600, 1, 100, 2, seed=3)))
    out.append(_seq("seq-long5", "", lambda: small_batch(400, 3, 100, 4, seed=10), q=_long_seq(5), small=False))
    for c in out:
        c.floor = c.floor or FLOORS.get(c.name, 0)
    return out


def _rising_seq(name):
    """_rising_runs (per-key v climbing in runs, rare drops and low w) at 400 rows over 2 keys: nearly every row lies
    inside an open sequence of seq_next, seq_or_next, seq_cross and seq_c3b (every count 1 .. 5 pending); the shapes
    whose last element needs a fall or a rise of w (seq_and, seq_count, seq_last_ref) match more on random values"""
    return _rising_runs(400, 2, seed=sum(name.encode()))


RISING = ("seq_next", "seq_or_next", "seq_cross", "seq_c3b")


# the growth stream of test_capacity.py: one key with 3,000 live partials through the per-key machine
GROWTH_ENGINE = dict(force_general=True, partial_lanes=-1)
GROWTH_CUT, GROWTH_EARLY = 1_700, 200


def growth_stream() -> Batch:
    return skewed(hot=3_000, cold=1_000)


# ---------------------------------------------------------------------------------------------- oracle, cuts, decoy
_WHOLE, _WANT, _CUTS = {}, {}, {}


def whole(case: SnapCase) -> Batch:
    if case.name not in _WHOLE:
        b = case.make()
        if not context(case.app).partitioned:
            b = Batch(b.n, b.base_index, b.ts, b.stream, np.zeros(b.n, np.int32), b.cols, b.nulls)
        _WHOLE[case.name] = b
    return _WHOLE[case.name]


def cat(outs) -> Outputs:
    return Outputs(*[np.concatenate([getattr(o, f) for o in outs]) for f in FIELDS])


def run_oracle(app, parts, fresh_each=False) -> Outputs:
    """the oracle over the pieces; fresh_each: a new engine per piece (an engine that forgets everything at a cut)"""
    ctx = context(app)
    outs, eng = [], None
    for p in parts:
        if eng is None or fresh_each:
            if eng is not None:
                eng.close()
            eng = OracleEngine(ctx)
        eng.push(p)
        outs.append(eng.fetch())
    eng.close()
    return cat(outs)


def want(case: SnapCase) -> Outputs:
    """the reference of every property: the oracle over the uninterrupted stream"""
    if case.name not in _WANT:
        _WANT[case.name] = run_oracle(case.app, [whole(case)])
    return _WANT[case.name]


def cover(out: Outputs, n: int) -> np.ndarray:
    """cover[c], c in 0 .. n: the matches that straddle a cut before row c (e1's row < c <= the trigger row)"""
    e1 = out.vals[:, 0].astype(np.int64)
    t = out.trigger.astype(np.int64)
    ok = (e1 < t) & (out.vnull[:, 0] == 0)
    d = np.zeros(n + 2, np.int64)
    np.add.at(d, e1[ok] + 1, 1)
    np.add.at(d, t[ok] + 1, -1)
    return np.cumsum(d)[:n + 1]


def place_cuts(case: SnapCase) -> List[int]:
    """Two rounds of the push sizes 1, 2, 3, 5, 8, 13, 21, 34 from a fifth into the stream, the nine deciles, the rows
    the case names and one adjacent pair (a 1-row push), each moved forward to the next cut some oracle match straddles.
    For the sequence shapes that is a trigger row of a match, as the cuts the case must have are."""
    n = whole(case).n
    cov = cover(want(case), n)
    good = np.flatnonzero(cov[1:n] > 0) + 1
    assert len(good) > 0, case.name

    def snap(c):
        i = int(np.searchsorted(good, c))
        return int(good[min(i, len(good) - 1)])
    targets, c = [n * k // 10 for k in range(1, 10)] + list(case.near), n // 5
    for s in STEPS * 2:
        c += s
        targets.append(c)
    cuts = {snap(t) for t in targets} | set(case.must_cut)
    pairs = good[:-1][np.diff(good) == 1]
    later = pairs[pairs >= n // 2]
    p = int(later[0] if len(later) else pairs[0])
    return sorted(cuts | {p, p + 1})


def cuts(case: SnapCase) -> List[int]:
    if case.name not in _CUTS:
        _CUTS[case.name] = place_cuts(case)
    return _CUTS[case.name]


def parts(case: SnapCase) -> List[Batch]:
    ps = V.pieces(whole(case), cuts(case))
    if case.sparse_nulls:
        for p in ps:
            p.nulls = [x if x is not None and x.any() else None for x in p.nulls]
    return ps


def _names(app):
    ctx = context(app)
    return [ctx.app.streams[ctx.stream_ids[s]].attrs[a][0] for s, a, t in L.column_layout(ctx)]


def key_count(case: SnapCase, b: Batch) -> int:
    """partition keys, or compared ids of an absence query, in b (1: the stream has no keys)"""
    if case.id_col is not None:
        live = b.stream == 0
        return len(np.unique(b.cols[case.id_col][live]))
    return len(np.unique(b.key))


def decoy(case: SnapCase) -> Batch:
    """The case's rows again as another stream: twice the keys (every key split in two by the row's parity), one day
    after the case's stream has ended, null flags (5 %) on every column but the partition key."""
    b = whole(case)
    n = b.n
    rng = np.random.default_rng(zlib.crc32(f"decoy/{case.name}".encode()))
    odd = (np.arange(n) % 2).astype(np.int32)
    partitioned = context(case.app).partitioned
    key = dense_first_seen(b.key * 2 + odd) if partitioned else b.key
    cols, nulls = [], []
    for k, (name, c) in enumerate(zip(_names(case.app), b.cols)):
        c = c.copy()
        if partitioned and name == "symbol":
            c = key.astype(c.dtype)
        elif case.id_col == k:
            c = (c * 2 + odd).astype(c.dtype)
        cols.append(c)
        nulls.append(None if name == "symbol" else (rng.random(n) < 0.05).astype(np.uint8))
    later = int(b.ts.max() - b.ts.min()) + DAY       # its first row lies a day after the case's last one
    return Batch(n, 0, b.ts + later, b.stream, key.astype(np.int32), cols, nulls)


def decoy_parts(case: SnapCase) -> List[Batch]:
    n = whole(case).n
    hb = np.flatnonzero(whole(case).stream == -1)
    edges = sorted({n // 3, 2 * n // 3} | {int(r) for r in hb} | {int(r) + 1 for r in hb if r + 1 < n})
    return V.pieces(decoy(case), [c for c in edges if 0 < c < n])


# ---------------------------------------------------------------------------------------------- drivers (GPU)
class Trace:
    """what a hop run delivered and, per push, the kernels the handle timed, the spilled units, whether the push ran
    on a restored handle and whether it was the first push of a handle that never held nulls"""

    def __init__(self):
        self.outs, self.log, self.restored, self.blobs = [], [], [], []

    def output(self) -> Outputs:
        return cat(self.outs)


def open_engine(case: SnapCase):
    from siddhi_amd._native import GpuEngine
    return GpuEngine(context(case.app), **case.engine)


def push(eng, piece: Batch, trace: Optional[Trace] = None, restored=False):
    """one push (a heartbeat row goes through sg_advance_time) and its fetch"""
    if piece.n == 1 and piece.stream is not None and piece.stream[0] == -1:
        eng.handle.advance_time(int(piece.ts[0]), int(piece.base_index))
    else:
        eng.push(piece)
    out = eng.fetch()
    if trace is not None:
        t = eng.handle.timing()
        trace.outs.append(out)
        trace.log.append(([name for name, _ in t.kernels()], int(t.spilled_units)))
        trace.restored.append(restored)
    return out


def hop_fresh(case: SnapCase, every=1) -> Trace:
    """after every push (every `every`-th cut): fetch, snapshot, close, open a new handle, restore"""
    tr, eng, restored = Trace(), open_engine(case), False
    ps = parts(case)
    for i, p in enumerate(ps):
        push(eng, p, tr, restored)
        if i + 1 < len(ps) and i % every == 0:
            blob = eng.snapshot()
            tr.blobs.append(blob)
            eng.close()
            eng = open_engine(case)
            eng.restore(blob)
            restored = True
    eng.close()
    return tr


def hop_ping_pong(case: SnapCase) -> Trace:
    """two handles opened once and never reset; the state hops A -> B -> A ..., so every restore lands on a handle that
    holds this stream's state from two cuts earlier"""
    tr, pair = Trace(), [open_engine(case), open_engine(case)]
    ps = parts(case)
    for i, p in enumerate(ps):
        cur, nxt = pair[i % 2], pair[(i + 1) % 2]
        push(cur, p, tr, i > 0)
        if i + 1 < len(ps):
            nxt.restore(cur.snapshot())
    for e in pair:
        e.close()
    return tr


def hop_decoy(case: SnapCase) -> Trace:
    """the target handle runs the decoy stream to its end, then takes the blob of the middle cut and runs the rest"""
    tr, src, dst = Trace(), open_engine(case), open_engine(case)
    ps = parts(case)
    mid = len(ps) // 2
    assert len(ps) - mid >= 3
    for p in decoy_parts(case):
        push(dst, p)
    for p in ps[:mid]:
        push(src, p, tr, False)
    dst.restore(src.snapshot())
    src.close()
    for p in ps[mid:]:
        push(dst, p, tr, True)
    dst.close()
    return tr


def hop_double(case: SnapCase) -> Trace:
    """at every cut: restore into X, snapshot X at once with nothing pushed, restore that blob into Y, continue on Y"""
    tr, eng = Trace(), open_engine(case)
    ps = parts(case)
    for i, p in enumerate(ps):
        push(eng, p, tr, i > 0)
        if i + 1 < len(ps):
            blob = eng.snapshot()
            eng.close()
            x = open_engine(case)
            x.restore(blob)
            again = x.snapshot()
            x.close()
            eng = open_engine(case)
            eng.restore(again)
    eng.close()
    return tr


HOPS = {"fresh": hop_fresh, "ping_pong": hop_ping_pong, "decoy": hop_decoy, "double_hop": hop_double}

CASES = cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# one case per state kind and lane mode
BLOB_CASES = ["carry-DOUBLE->-stack", "once-LONG->-split", "absent-filters", "machine-c3c", "lanes-count13",
              "seq-seq_c3b", "seq-long5"]
