"""Apps, rows and comparison helpers shared by the range routing tests (test_range_reference.py on the CPU,
test_range_router.py on the GPU).  Expected values come from range_ref.route; this module only builds inputs and
compares a routed Batch with them."""
import functools
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))

import range_ref  # noqa: E402
from oracle import OracleEngine  # noqa: E402  (checker engine; CPU)
from siddhi_amd import SiddhiManager, StreamCallback  # noqa: E402
from siddhi_amd import compiler as C  # noqa: E402
from siddhi_amd.runtime import Batch  # noqa: E402

NP = {"STRING": np.int32, "INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64,
      "BOOL": np.int32}

# ------------------------------------------------------------------------------------------- the all-type stream
ATTRS = [("s", "STRING"), ("i", "INT"), ("l", "LONG"), ("f", "FLOAT"), ("d", "DOUBLE"), ("b", "BOOL"),
         ("i2", "INT"), ("l2", "LONG"), ("f2", "FLOAT"), ("d2", "DOUBLE")]
TYPED = ("define stream S (" + ", ".join(f"{n} {t.lower()}" for n, t in ATTRS) + "); "
         "partition with ({} of S) begin @info(name='q') from every e1=S -> e2=S[i>e1.i] "
         "select e1.i as a insert into M; end;")
NUMERIC_COLS = [n for n, t in ATTRS if t in range_ref.NUMERIC]
OPS = ("==", "!=", ">", ">=", "<", "<=")
CONSTANTS = ("16777217", "9007199254740993l", "16777216.0f", "0.0", "2147483647")

INT_MIN, INT_MAX = -2**31, 2**31 - 1
LONG_MIN, LONG_MAX = -2**63, 2**63 - 1
NAN, INF = float("nan"), float("inf")
F = range_ref.f32
# The edge values around which a compare in the wrong domain gives another answer: 2^24 + 1 is the first integer a
# binary32 cannot hold, 2^53 + 1 the first a binary64 cannot, 2^60 + 2^36 + 1 rounds to 2^60 + 2^37 as a binary32 in
# one step and to 2^60 through a double, LONG_MAX becomes 2^63 in either.  Beyond the bare edges every pool holds the
# values the constants of CONSTANTS need so that `column == constant` holds somewhere (2^24 and INT_MAX among the
# longs, 2^31 and 2^53 among the floats, 2^24 among the doubles).
POOLS = {
    "INT": [INT_MIN, -1, 0, 1, 2, 2**24, 2**24 + 1, INT_MAX],
    "LONG": [LONG_MIN, -(2**53) - 1, -1, 0, 2, 2**24, 2**24 + 1, INT_MAX, 2**53, 2**53 + 1, 2**60 + 2**36 + 1,
             LONG_MAX],
    "FLOAT": [NAN, INF, -INF, 0.0, -0.0, 1.5, 2.0, 2.0**24, 2.0**31, 2.0**53, 2.0**60, F(3.4e38), F(1e-45), 2.0**63],
    "DOUBLE": [NAN, INF, -INF, 0.0, -0.0, 0.5, 2.0, 2.0**24, 2.0**24 + 1, 2.0**53, 2.0**63, 1e308, 2147483647.0],
    "STRING": ["abc", "x0", "x2", ""],
    "BOOL": [True, False],
}


def pair_conditions():
    """every ordered pair of numeric columns x the six operators"""
    return [f"{a}{op}{b}" for a in NUMERIC_COLS for b in NUMERIC_COLS if a != b for op in OPS]


def constant_conditions():
    """every numeric column x the edge constants x the six operators (i2 and d2 never carry a null array, so the
    constant compares also run on a column without one), and each constant once on the left"""
    out = [f"{c}{op}{k}" for c in NUMERIC_COLS for k in CONSTANTS for op in OPS]
    left = zip(CONSTANTS, ("==", "<", ">=", "!=", ">"), ("l", "f", "d", "f2", "l2"))
    return out + [f"{k}{op}{c}" for k, op, c in left]


OTHER = [
    "s=='abc'", "s!='abc'", "'abc'==s", "s==''", "s=='never sent'", "s!='never sent'",     # STRING, one never sent
    "b==true", "b!=true", "b==false", "false!=b", "b", "not b",                            # BOOL
] + [f"{n} is null" for n, _ in ATTRS] + [f"not ({n} is null)" for n, _ in ATTRS]
# the forms of test_range_router.CONDITIONS that are no plain pair of columns (those are in pair_conditions), and
# `is null` of a non-BOOL attribute inside and / or / not
NESTED = [
    "i>0 and f<3.0", "(i<0 or d>0.7)", "not (l>1l)", "i!=2", "f!=1.5f",
    "(i>0 and (f<3.0 or d>1.0)) and not (l==2l or b)",
    "not (l is null) and i>0", "(f is null or d is null)", "s is null and not (b is null)",
    "(i>0 and (f is null or l2<=f)) and not (s=='abc' or d2 is null)", "i>1", "l<=2l", "f>=2.5f", "d<0.5",
]
# Conditions that are constant over every row whatever the pools hold, with their value: the string no row carries; an
# INT against 2^53 + 1 (as LONG) or above INT_MAX, which no int reaches (on i, < and <= still fail on a null row and !=
# holds on it too; i2 has no null row, so there they hold on every row); and `is null` of the two columns that never
# carry a null array.
CONSTANT_BY_DESIGN = {
    "s=='never sent'": False, "s!='never sent'": True,
    "i==9007199254740993l": False, "i>9007199254740993l": False, "i>=9007199254740993l": False,
    "i!=9007199254740993l": True, "i>2147483647": False,
    "i2==9007199254740993l": False, "i2>9007199254740993l": False, "i2>=9007199254740993l": False,
    "i2!=9007199254740993l": True, "i2<9007199254740993l": True, "i2<=9007199254740993l": True,
    "i2>2147483647": False, "i2<=2147483647": True,
    "i2 is null": False, "d2 is null": False, "not (i2 is null)": True, "not (d2 is null)": True,
}


def all_conditions():
    return pair_conditions() + constant_conditions() + OTHER + NESTED


def typed_apps():
    """the conditions split into apps of at most 32 ranges (the nested forms 7 to an app: an app's programs share
    512 code words): [(app text, [condition, ...])]; label r<k> = the k-th range"""
    flat = pair_conditions() + constant_conditions() + OTHER
    parts = [flat[lo:lo + 32] for lo in range(0, len(flat), 32)]
    parts += [NESTED[lo:lo + 7] for lo in range(0, len(NESTED), 7)]
    return [(TYPED.format(" or ".join(f"{c} as 'r{k}'" for k, c in enumerate(part))), part) for part in parts]


def typed_rows(n, seed, null_rate=0.15):
    """n rows of S drawn from the pools, about 15 % nulls on every column but i2 and d2 (so some columns never carry a
    null array)"""
    rng = np.random.default_rng(seed)
    draws = []
    for name, t in ATTRS:
        pool = POOLS[t]
        pick = rng.integers(0, len(pool), n)
        isnull = rng.random(n) < (0.0 if name in ("i2", "d2") else null_rate)
        draws.append([None if isnull[r] else pool[pick[r]] for r in range(n)])
    ts = np.cumsum(rng.integers(0, 4, n))
    return [(0, int(ts[r]), [col[r] for col in draws]) for r in range(n)]


# ------------------------------------------------------------------------------------------- rows <-> batches
def batch_of(app: C.SiddhiApp, rows, strings: dict, base=0, keys=None, index=None, value_key=None):
    """rows (range_ref's form) as the runtime's SoA Batch: one column per attribute of every stream (zero outside the
    row's stream and under a null), a null array where the column has a null, string ids from `strings` (grown as
    needed).  keys / value_key: dictionary and per-stream key attribute for rows of value-partitioned streams."""
    n = len(rows)
    sids = list(app.streams.keys())
    cols, nulls = [], []
    for s, sid in enumerate(sids):
        for a, (_, t) in enumerate(app.streams[sid].attrs):
            col, nul = np.zeros(n, NP[t]), None
            for r, (rs, _, v) in enumerate(rows):
                if rs != s:
                    continue
                x = v[a]
                if x is None:
                    nul = np.zeros(n, np.uint8) if nul is None else nul
                    nul[r] = 1
                elif t == "STRING":
                    col[r] = strings.setdefault(x, len(strings))
                else:
                    col[r] = x
            cols.append(col)
            nulls.append(nul)
    key = np.full(n, -1, np.int32)
    for r, (rs, _, v) in enumerate(rows):
        if value_key and rs in value_key:
            key[r] = keys[str(v[value_key[rs]])]
    return Batch(n, base, np.array([t for _, t, _ in rows], np.int64), np.array([s for s, _, _ in rows], np.int32), key,
                 cols, nulls, index=index)


def _bits(t, x):
    if t == "FLOAT":
        return struct.pack("<f", x)
    if t == "DOUBLE":
        return struct.pack("<d", x)
    return x


def assert_routed(got: Batch, want: range_ref.Routed, b: Batch, app: C.SiddhiApp, strings: dict, what=""):
    """every field of the routed batch equals the reference's copies: index, stream, key, timestamp; the values of the
    copy's own stream (bit for bit, null for null) from the reference's tuples; and every column and null array, the
    other streams' included, is the input's gathered through the reference's source rows"""
    assert got.n == len(want.rows), what
    index = got.index if got.index is not None else np.uint64(got.base_index) + np.arange(got.n, dtype=np.uint64)
    assert index.tolist() == [r[0] for r in want.rows], what
    assert got.stream.tolist() == [r[1] for r in want.rows], what
    assert got.key.tolist() == [r[2] for r in want.rows], what
    assert got.ts.tolist() == [r[3] for r in want.rows], what
    src = np.array(want.src, np.int64)
    for c in range(len(b.cols)):
        assert got.cols[c].dtype == b.cols[c].dtype and got.cols[c].tobytes() == b.cols[c][src].tobytes(), (what, c)
        assert (got.nulls[c] is None) == (b.nulls[c] is None), (what, c)
        if got.nulls[c] is not None:
            assert np.array_equal(got.nulls[c], b.nulls[c][src]), (what, c)
    sids = list(app.streams.keys())
    back = {i: s for s, i in strings.items()}
    cb = np.cumsum([0] + [len(app.streams[sid].attrs) for sid in sids])
    for k in range(0, len(want.rows), 1 if len(want.rows) < 500 else 37):     # (a sample of a long batch)
        values = want.rows[k][4]
        s = int(b.stream[want.src[k]])
        if values is None:
            continue
        for a, (_, t) in enumerate(app.streams[sids[s]].attrs):
            c = int(cb[s]) + a
            if got.nulls[c] is not None and got.nulls[c][k]:
                v = None
            else:
                v = got.cols[c][k].item()
                v = back[v] if t == "STRING" else bool(v) if t == "BOOL" else v
            assert (v is None) == (values[a] is None), (what, k, a)
            if v is not None:
                assert _bits(t, v) == _bits(t, values[a]), (what, k, a)


# ------------------------------------------------------------------------------------------- typed cases
N_ROWS = 2000
TYPED_APPS = typed_apps()


class Case:
    """one typed app: its rows and the reference's routing of them.  Only these are shared between tests (typed_case
    caches them) and no test changes them; a test that needs a runtime opens its own with runtime()."""

    def __init__(self, text, conds, seed, n=N_ROWS, base=500):
        self.text, self.conds, self.n, self.base = text, conds, n, base
        self.rows = typed_rows(n, seed)
        self.want = range_ref.route(C.parse(text), self.rows, base_index=base)

    def runtime(self):
        """(a fresh oracle-engine runtime of the app, the rows as a Batch of it); the caller shuts the runtime down"""
        rt = SiddhiManager(engine=OracleEngine).createSiddhiAppRuntime(self.text)
        return rt, batch_of(rt.app, self.rows, rt.strings, base=self.base)

    def masks(self):
        """per range, the rows the reference sent to it (label r<k> = range k)"""
        m = np.zeros((len(self.conds), self.n), bool)
        for (_, _, key, _, _), src in zip(self.want.rows, self.want.src):
            m[int(self.want.keys[key][1:]), src] = True
        return m


@functools.lru_cache(maxsize=None)
def typed_case(k):
    return Case(TYPED_APPS[k][0], TYPED_APPS[k][1], 100 + k)


# ------------------------------------------------------------------------------------------- `is null` of any type
IS_NULL = ["price is null as 'missing'",
           "not (price is null) as 'there' or symbol is null as 'anon'",
           "price is null and volume>0 as 'a' or (volume is null or price<20) as 'b' or "
           "not (symbol is null) and price>=20 as 'c'"]


def price_rows(n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n):
        v = [None if rng.random() < 0.2 else f"s{int(rng.integers(0, 3))}",
             None if rng.random() < 0.3 else float(np.float32(rng.integers(10, 80) / 2)),
             None if rng.random() < 0.2 else int(rng.integers(-2, 3))]
        rows.append((0, 3 * r, v))
    return rows


# ------------------------------------------------------------------------------------------- flush granularity
MIXED3 = ("define stream S (k int); define stream T (v int); define stream G (g int); "
          "partition with (k of S, v>0 as 'L' of T) begin from every e1=G -> e2=S or e3=T "
          "select e1.g as g, e2.k as k, e3.v as v insert into M; end;")
MIXED = ("define stream S (k int); define stream T (v int); define stream G (g int); "
         "partition with (k of S, v>0 as 'L' or v>100 as 'M' or v<0 as 'N' or v>-5 as '7' of T) begin "
         "from every e1=G -> e2=S or e3=T select e1.g as g, e2.k as k, e3.v as v insert into M; end;")


def mixed_rows(n, seed, rate=0.1):
    """S, T and G rows in random order; the value keys and the labels come in one after another (a new one about
    every 1 / rate rows), so most of them first appear after some G row.  Label '7' is also a value key: one
    instance."""
    rng = np.random.default_rng(seed)
    rows, nk = [], 1
    for r in range(n):
        nk += rng.random() < rate
        s = int(rng.integers(0, 3))
        if s == 0:
            v = int(rng.integers(1, nk + 1)) + 5
        elif s == 1:
            v = int([3, 3, -7, 150, -2, 0][int(rng.integers(0, min(6, nk)))])
        else:
            v = r
        rows.append((s, 2 * r, [v]))
    return rows


def run_flushed(engine, text, rows, cuts):
    """send the rows, flushing after every row position in `cuts`: (delivered rows, dictionary in creation order, the
    (index, stream, key, ts) of every row the engine was pushed)"""
    rt = SiddhiManager(engine=engine).createSiddhiAppRuntime(text)
    got, pushed = [], []

    class CB(StreamCallback):
        def receive(self, events):
            got.extend((e.timestamp, tuple(e.data)) for e in events)

    rt.addCallback("M", CB())
    rt.start()
    eng = rt.queries[0].engine
    inner = eng.push

    def recording_push(b):
        index = range(b.base_index, b.base_index + b.n) if b.index is None else b.index.tolist()
        pushed.extend(zip(index, b.stream.tolist(), b.key.tolist(), b.ts.tolist()))
        inner(b)
    eng.push = recording_push
    hs = [rt.getInputHandler(sid) for sid in rt.stream_ids]
    for r, (s, ts, v) in enumerate(rows):
        hs[s].send(ts, v)
        if r in cuts:
            rt.flush()
    rt.flush()
    keys = list(rt.key_dicts[0])
    rt.shutdown()
    return got, keys, pushed


def flush_plans(n, seed=1, every_row=True, pieces=None):
    rng = np.random.default_rng(seed)
    plans = {"one flush": set(),
             "random split": set(rng.choice(n, max(1, n // 12 if pieces is None else pieces), replace=False).tolist())}
    if every_row:
        plans["every row"] = set(range(n))
    return plans


def check_flush_granularity(engine, text, rows, min_delivered=0, plans=None, delivered=None):
    """however the rows are flushed, the engine is pushed the reference router's copies, the dictionary is created in
    the reference's order and the same rows are delivered (`delivered`, or what the first plan delivered)"""
    want = range_ref.route(C.parse(text), rows)
    plans = flush_plans(len(rows)) if plans is None else plans
    runs = {name: run_flushed(engine, text, rows, cuts) for name, cuts in plans.items()}
    delivered = next(iter(runs.values()))[0] if delivered is None else delivered
    for name, (got, keys, pushed) in runs.items():
        assert keys == want.keys, name
        assert pushed == [r[:4] for r in want.rows], name
        assert got == delivered, name
    assert len(delivered) >= min_delivered
    return delivered
