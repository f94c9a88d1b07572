"""The cases of test_value_cases.py (CPU guard), test_closed_form_values.py and test_pred_pass.py (GPU): compared values
from edge pools on every route of the every-next closed form and of the once route, and filter constants on rounding
edges through both predicate kernels.  Pure numpy; importable without a GPU.

Every case is a query text, one stream of rows (numpy columns in the batch layout) and the cuts at which it is pushed;
`reference()` runs the row-at-a-time restatement (closed_form_ref.py) over the same rows as Python scalars."""
import dataclasses
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List, Optional

import numpy as np

import closed_form_ref as R
import range_ref
from parity_util import context, dense_first_seen
from siddhi_amd import compiler as C
from siddhi_amd import lowering as L
from siddhi_amd.runtime import Batch

T0 = 1_700_000_000_000
NP = {"INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64}
TYPES = ("INT", "LONG", "FLOAT", "DOUBLE")
OPS = (">", ">=", "<", "<=")
OPS6 = ("==", "!=", ">", ">=", "<", "<=")

F32_01 = float(np.float32(0.1))
POOLS = {
    "INT": [-2**31, -2**31 + 1, -1, 0, 1, 1, 7, 7, -7, 2**24, 2**24 + 1, 2**31 - 2, 2**31 - 1],
    "LONG": [-2**63, -2**63 + 1, -2**53 - 1, -2**53, -1, 0, 1, 1, 7, 7, 2**31, 2**32, 2**53, 2**53 + 1, 2**53 + 2,
             2**60 + 2**36 + 1, 2**63 - 2, 2**63 - 1],
    "FLOAT": [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1, 1, -1, 2.5, 2.5, 3e38, -3e38, 2.0**24, 2.0**24 + 2],
    "DOUBLE": [np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1, 1, -1, 2.5, 2.5, 1e308, -1e308, 2.0**53,
               2.0**53 + 2, F32_01, 0.1],
}
# the predicate cases' columns: the pools above and the values around 2^24 a binary32 cannot tell apart
PRED_POOLS = {
    "INT": POOLS["INT"] + [2**24, 2**24 + 1, 2**24 + 2],
    "FLOAT": POOLS["FLOAT"] + [2.0**24, 2.0**24 + 2, F32_01],
}


def pool_array(typ, pool=None):
    return np.array(POOLS[typ] if pool is None else pool, dtype=NP[typ])


@dataclass
class Case:
    name: str
    kind: str                     # "every" / "once" (closed forms) / "filter" (general family, P1)
    app: str
    typ: str
    op: str
    n: int
    keys: int                     # 0: unpartitioned
    step_ms: int
    seed: int
    cuts: List[int] = field(default_factory=list)
    route: str = ""
    engine: dict = field(default_factory=dict)      # GpuEngine keywords
    shift_from: Optional[int] = None                # rows from here on lie 3,000,000,000 ms later
    time_back: bool = False                         # every row with i % 97 == 5 lies 400 ms earlier
    streams: int = 1
    null_frac: float = 0.03
    null_streams: Optional[tuple] = None            # streams whose compared column has nulls (None: every stream)
    pool: Optional[list] = None
    floor: int = 300
    no_stream_column: bool = False                  # the GPU test also pushes the batch without a stream column

    def __str__(self):
        return self.name


# ---------------------------------------------------------------------------------------------- rows
@lru_cache(maxsize=None)
def _context(app):
    return context(app)


def batch(case: Case) -> Batch:
    """the case's whole stream as one batch: id = row number, symbol = key id, the compared attributes from the pool
    with nulls, every other INT attribute uniform in [0, 1000)"""
    ctx = _context(case.app)
    rng = np.random.default_rng(case.seed)
    n = case.n
    ts = T0 + case.step_ms * np.arange(n, dtype=np.int64)
    if case.shift_from is not None:
        ts[case.shift_from:] += 3_000_000_000
    if case.time_back:
        ts[np.arange(n) % 97 == 5] -= 400
    key = rng.integers(0, case.keys, n).astype(np.int32) if case.keys else np.zeros(n, np.int32)
    stream = rng.integers(0, case.streams, n).astype(np.int32)
    pool = pool_array(case.typ, case.pool)
    cols, nulls = [], []
    for s, a, t in L.column_layout(ctx):
        name = ctx.app.streams[ctx.stream_ids[s]].attrs[a][0]
        nul = None
        if name == "id":
            c = np.arange(n, dtype=np.int64)
        elif name == "symbol":
            c = key.copy()
        elif name in ("v", "x", "y", "price"):
            c = pool[rng.integers(0, len(pool), n)]
            if case.null_frac and (case.null_streams is None or s in case.null_streams):
                nul = (rng.random(n) < case.null_frac).astype(np.uint8)
        else:
            c = rng.integers(0, 1000, n).astype(np.int32)
        cols.append(c)
        nulls.append(nul)
    if case.keys:   # dense ids in first-seen order, as the runtime's key dictionary hands them out
        key = dense_first_seen(key)
    return Batch(n, 0, ts, stream, key, cols, nulls)


def pieces(b: Batch, cuts, stream_column=True) -> List[Batch]:
    out, lo = [], 0
    for hi in list(cuts) + [b.n]:
        out.append(Batch(hi - lo, b.base_index + lo, b.ts[lo:hi], b.stream[lo:hi] if stream_column else None,
                         b.key[lo:hi], [np.ascontiguousarray(c[lo:hi]) for c in b.cols],
                         [None if x is None else np.ascontiguousarray(x[lo:hi]) for x in b.nulls]))
        lo = hi
    return out


def pushes(case: Case, stream_column=True) -> List[Batch]:
    return pieces(batch(case), case.cuts, stream_column)


def _scalar(x, t):
    if t in ("INT", "LONG", "STRING"):
        return int(x)
    return float(x)         # a binary32 widens exactly


def ref_rows(case: Case, b: Optional[Batch] = None):
    """(stream, ts, key, values) per row, values over the attributes of the row's stream, None for a null"""
    ctx = _context(case.app)
    b = batch(case) if b is None else b
    layout = L.column_layout(ctx)
    by_stream = {}
    for c, (s, a, t) in enumerate(layout):
        by_stream.setdefault(s, []).append((c, t))
    rows = []
    for r in range(b.n):
        s = int(b.stream[r])
        values = [None if (b.nulls[c] is not None and b.nulls[c][r]) else _scalar(b.cols[c][r], t)
                  for c, t in by_stream[s]]
        rows.append((s, int(b.ts[r]), int(b.key[r]) if ctx.partitioned else 0, values))
    return rows


# ---------------------------------------------------------------------------------------------- the pattern, from the AST
def _conjuncts(e, out):
    if isinstance(e, C.And):
        _conjuncts(e.left, out)
        _conjuncts(e.right, out)
    else:
        out.append(e)
    return out


def _reads(e, ref) -> bool:
    if isinstance(e, C.Var):
        return e.stream_ref == ref
    return any(_reads(getattr(e, f), ref) for f in getattr(e, "__dataclass_fields__", ()) if f != "op")


FLIP = {">": "<", ">=": "<=", "<": ">", "<=": ">="}


def pattern(case: Case):
    """(every?, A side, B side, op of `B.x OP A.x`, within) read off the parsed query"""
    ctx = _context(case.app)
    q = ctx.query
    el = q.input.element
    assert isinstance(el, C.NextStateElement)
    first, second = el.current, el.next
    every = isinstance(first, C.EveryStateElement)
    if every:
        first = first.inner
    da, db = ctx.app.streams[first.stream_id], ctx.app.streams[second.stream_id]
    conj = []
    for f in second.filters:
        _conjuncts(f, conj)
    cross = [c for c in conj if _reads(c, first.ref)]
    local = [c for c in conj if not _reads(c, first.ref)]
    op, attr_a, attr_b = None, 0, 0
    if cross:
        (c,) = cross
        op, l, r = c.op, c.left, c.right
        if l.stream_ref == first.ref:
            op, l, r = FLIP[op], r, l
        attr_a, attr_b = da.attr_index(r.attr), db.attr_index(l.attr)
    a = R.Side(ctx.stream_index(first.stream_id), da, attr_a, list(first.filters))
    b = R.Side(ctx.stream_index(second.stream_id), db, attr_b, local)
    return every, a, b, op, q.input.within


_ROWS = {}


def _rows_cached(case: Case):
    """the case's rows as Python scalars, made once per case (names are unique)"""
    if case.name not in _ROWS:
        _ROWS[case.name] = ref_rows(case)
    return _ROWS[case.name]


def reference(case: Case, compare=range_ref._compare, expired=None):
    """the reference's (trigger, e1, e2) triples over the case's whole stream"""
    every, a, b, op, within = pattern(case)
    rows = _rows_cached(case)
    kw = {} if expired is None else {"expired": expired}
    if case.kind == "filter":
        keep = [i for i, (s, _, _, v) in enumerate(rows) if s == a.stream and
                all(R.holds(e, a.defn, v, compare) for e in a.conds)]
        return [(i + 1, i, i + 1) for i in keep if i + 1 < len(rows)]
    fn = R.every_next if every else R.once
    return fn(rows, a, b, op, within, _context(case.app).partitioned, compare, **kw)


def triples(out) -> list:
    """(trigger, e1.id, e2.id) of an engine's output whose select begins `e1.id, e2.id`"""
    return list(zip(out.trigger.astype(np.int64).tolist(), out.vals[:, 0].tolist(), out.vals[:, 1].tolist()))


# ---------------------------------------------------------------------------------------------- queries
def _t(typ):
    return typ.lower()


def q_one(typ, op, every=True, partitioned=True, list_mode=False):
    cond = f"v {op} e1.v" + (" and w > 300" if list_mode else "")
    body = (f"@info(name='q') from {'every ' if every else ''}e1=S[w >= 100] -> e2=S[{cond}] within 1 sec "
            "select e1.id as i1, e2.id as i2, e1.v as v1, e2.v as v2 insert into M;")
    head = f"define stream S (id long, symbol string, v {_t(typ)}, w int); "
    return head + (f"partition with (symbol of S) begin {body} end;" if partitioned else body)


def q_two(typ, op):
    return (f"define stream A (id long, symbol string, x {_t(typ)}, w int); "
            f"define stream B (id long, symbol string, y {_t(typ)}, w int); "
            "partition with (symbol of A, symbol of B) begin @info(name='q') "
            f"from every e1=A[w >= 100] -> e2=B[y {op} e1.x] within 1 sec "
            "select e1.id as i1, e2.id as i2, e1.x as v1, e2.y as v2 insert into M; end;")


def _seed(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name)) % 100_000


def _case(name, kind, app, typ, op, n, keys, step, **kw):
    return Case(name, kind, app, typ, op, n, keys, step, kw.pop("seed", _seed(name)), **kw)


def closed_form_cases() -> List[Case]:
    out = []
    for typ in TYPES:
        for op in OPS:                       # tiled walker: every type x every operator x stack / list mode
            for mode in ("stack", "list"):
                out.append(_case(f"tiled-{typ}-{op}-{mode}", "every", q_one(typ, op, list_mode=mode == "list"), typ, op,
                                 6000, 40, 50, route="tiled", no_stream_column=True))
        for op in (">", "<="):
            P = dict(n=6000, keys=40, step=50)
            U = dict(n=3000, keys=0, step=5)
            G = dict(n=3000, keys=25, step=50, floor=200)
            tag = f"{typ}-{op}"
            out.append(_case(f"sorted-{tag}", "every", q_one(typ, op), typ, op, **P, route="sorted",
                             engine={"partition_sort": 1}))
            out.append(_case(f"search-{tag}", "every", q_one(typ, op, partitioned=False), typ, op, **U, route="search"))
            out.append(_case(f"flat_walker-{tag}", "every", q_one(typ, op, partitioned=False), typ, op, **U,
                             route="flat_walker", engine={"walker_only": True}))
            for mode in ("stack", "list"):
                lm = mode == "list"
                out.append(_case(f"redo-{tag}-{mode}", "every", q_one(typ, op, list_mode=lm), typ, op, **P, route="redo",
                                 engine={"ring_cap": 2}))
                out.append(_case(f"carry-{tag}-{mode}", "every", q_one(typ, op, list_mode=lm), typ, op, **P,
                                 route="carry", cuts=[1, 3000, 3001]))
            out.append(_case(f"wide-{tag}-one_push", "every", q_one(typ, op), typ, op, **G, route="wide",
                             shift_from=1500))
            out.append(_case(f"wide-{tag}-pushes", "every", q_one(typ, op), typ, op, **G, route="wide", shift_from=1500,
                             cuts=[700, 1500, 1501]))
            out.append(_case(f"time_back-{tag}", "every", q_one(typ, op), typ, op, **G, route="time_back",
                             time_back=True))
            # (two streams halve the rows that can start or complete a partial: at 6,000 rows `>` on FLOAT and DOUBLE
            # stays under the floor of 300 matches for every seed in 1 .. 399; 8,000 rows reach it)
            out.append(_case(f"two_streams-{tag}", "every", q_two(typ, op), typ, op, n=8000, keys=40, step=50,
                             route="two_streams", streams=2))
        for op in OPS:                       # the once route, in one push and split in two
            for cuts in ([], [1500]):
                out.append(_case(f"once-{typ}-{op}-{'split' if cuts else 'one_push'}", "once",
                                 q_one(typ, op, every=False), typ, op, 3000, 300, 2, route="once", cuts=cuts, floor=100))
    return out


# ---------------------------------------------------------------------------------------------- predicate cases
PRED_SIZES = [1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4099]     # consecutive batches of one engine
PRED_N = sum(PRED_SIZES)
PRED_CUTS = list(np.cumsum(PRED_SIZES)[:-1])

# constant per (column type, constant type), each on a rounding edge
CONSTANTS = {
    "INT": ["16777217", "2147483648L", "16777216.0f", "16777216.5"],
    "FLOAT": ["16777217", "16777217L", "0.1f", "0.1", "-0.0"],
}
LEFT_CONSTANT = "16777217L <= v"


def _cname(c):
    return c.replace(".", "p").replace("-", "m")


def q_p1(typ, cond):
    return (f"define stream S (id long, symbol string, v {_t(typ)}, w int); @info(name='q') "
            f"from every e1=S[{cond}] -> e2=S select e1.id as i1, e2.id as i2 insert into M;")


def q_p2(typ, cond):
    return (f"define stream S (id long, symbol string, v {_t(typ)}, w int); @info(name='q') "
            f"from every e1=S[{cond}] -> e2=S[v >= e1.v] within 10 sec "
            "select e1.id as i1, e2.id as i2, e1.v as v1, e2.v as v2 insert into M;")


def q_p3(cond):
    return ("define stream A (id long, symbol string, price float); "
            "define stream B (id long, symbol string, price float); @info(name='q') "
            f"from every e1=A[{cond}] -> e2=B[price > e1.price] within 10 sec "
            "select e1.id as i1, e2.id as i2, e1.price as v1, e2.price as v2 insert into M;")


def q_p4(cond):
    return ("define stream A (id long, symbol string, price float); "
            "define stream B (id long, symbol string, price float); "
            "partition with (symbol of A, symbol of B) begin @info(name='q') "
            f"from e1=A[{cond}] -> e2=B[price > e1.price] "
            "select e1.id as i1, e2.id as i2, e1.price as v1, e2.price as v2 insert into M; end;")


def _pred(name, kind, app, typ, op, keys=0, **kw):
    return _case(name, kind, app, typ, op, PRED_N, keys, 5, cuts=PRED_CUTS, pool=PRED_POOLS[typ], floor=0, **kw)


def predicate_cases() -> List[Case]:
    """P1 / P2 / P3 / P4; the nulls of the compared column are the test's choice (null_frac here is the with-nulls run)"""
    out = []
    for typ in ("INT", "FLOAT"):
        conds = [(f"{_cname(c)}-{op}", f"v {op} {c}", op, c) for c in CONSTANTS[typ] for op in OPS6]
        conds.append(("left_constant", LEFT_CONSTANT, "<=", "left"))
        for tag, cond, op, c in conds:      # (one stream of rows per constant: the six operators see the same rows)
            seed = _seed(typ + c)
            out.append(_pred(f"P1-{typ}-{tag}", "filter", q_p1(typ, cond), typ, op, null_frac=0.05, seed=seed))
            out.append(_pred(f"P2-{typ}-{tag}", "every", q_p2(typ, cond), typ, op, null_frac=0.05, seed=seed))
    # two streams: nulls in A's price only -- k_pred_simple_s needs B's compared column without a null array
    for c in ("16777217", "0.1f", "0.1"):
        for op in OPS6:
            out.append(_pred(f"P3-{_cname(c)}-{op}", "every", q_p3(f"price {op} {c}"), "FLOAT", op, null_frac=0.05,
                             null_streams=(0,), streams=2, seed=_seed("P3" + c)))
    for c in ("0.1f", "0.1"):       # the once route's predicate pass: a null price passes `!=` and binds e1
        for op in OPS6:
            out.append(_pred(f"P4-{_cname(c)}-{op}", "once", q_p4(f"price {op} {c}"), "FLOAT", op, keys=600,
                             null_frac=0.05, null_streams=(0,), streams=2, seed=_seed("P4" + c)))
    return out


def without_nulls(case: Case) -> Case:
    return dataclasses.replace(case, name=case.name + "-no_nulls", null_frac=0.0)


# VM depth: right-nested `and (.. or (..))` compares; the bucket is the register stack k_pred<D> picks
def nested(k):
    """a filter of k compares: c1 and (c2 or (c3 and (c4 or ...)))"""
    cmps = [f"v {('>', '<=', '==', '>=', '<', '!=')[j % 6]} {(7, 0, 1, 16777217, -7)[j % 5]}" if j % 3 else
            f"w {OPS[j % 4]} {300 + 37 * j}" for j in range(k)]
    e = cmps[-1]
    for j in range(k - 2, -1, -1):
        e = f"{cmps[j]} {'and' if j % 2 == 0 else 'or'} ({e})"
    return e


DEPTH_BUCKETS = [(0, 2), (2, 4), (4, 8), (8, 16)]
DEPTH_COMPARES = [1, 3, 6, 12]


def depth_cases() -> List[Case]:
    return [_pred(f"depth-{k}", "filter", q_p1("INT", nested(k)), "INT", "or", null_frac=0.05) for k in DEPTH_COMPARES]


CLOSED = closed_form_cases()
PRED = predicate_cases()
DEPTH = depth_cases()
BY_NAME = {c.name: c for c in CLOSED + PRED + DEPTH}
assert len(BY_NAME) == len(CLOSED) + len(PRED) + len(DEPTH)


# ---------------------------------------------------------------------------------------------- GPU side
def run_gpu(case: Case, stream_column=True):
    """(output, [(kernel names, spilled units) per push]) of the GPU engine over the case's pushes"""
    from parity_util import run_engine
    from siddhi_amd._native import GpuEngine
    log = []

    class Witness(GpuEngine):
        """records, per push, the names of the kernels the handle timed and the spilled units"""

        def __init__(self, ctx):
            super().__init__(ctx, **case.engine)

        def push(self, b):
            super().push(b)
            t = self.handle.timing()
            log.append(([name for name, _ in t.kernels()], int(t.spilled_units)))

    got = run_engine(Witness, case.app, pushes(case, stream_column))
    return got, log
