"""Cases of range partitions through the node pipeline (sg_node_set_ranges), shared by test_node_ranges.py (GPU) and
test_node_range_cases.py (CPU, which guards the cases themselves).

Every expectation comes from range_ref.route (a row-at-a-time restatement that shares no code with either product
router): the rows are routed there, the oracle engine runs over the routed copies (dense ids in creation order, the
event's index on every copy), and the node's delivered columns must equal the oracle's outputs.  A case chooses the raw
64-bit key of every label and value-key string itself (Case.raw), with the Python mix64 of siddhi_amd/router.py, so that
labels one event holds together live on different shards where the case says so."""
import functools
import os
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))

import range_cases as RC  # noqa: E402
import range_ref  # noqa: E402
from oracle import OracleEngine  # noqa: E402  (checker engine; CPU)
from siddhi_amd import compiler as C  # noqa: E402
from siddhi_amd import lowering as L  # noqa: E402
from siddhi_amd.router import mix64  # noqa: E402
from siddhi_amd.runtime import Batch, Outputs  # noqa: E402
from test_range_partition import RANGES, _random_rows, app  # noqa: E402

FIELDS = ("trigger", "ts", "key", "group", "vals", "vnull")


def shard(raw: int, gpus: int) -> int:
    return int(mix64(np.array([raw], np.int64))[0] % np.uint64(gpus))


def spread(names, apart, gpus=(2, 3, 4), first=1000):
    """name -> raw key: small integers picked so that every pair in `apart` lives on different shards at every G of
    `gpus` (a deterministic search over mix64: the same raws on every run)"""
    raw, cand = {}, first
    for n in names:
        while True:
            ok = cand not in raw.values()
            for a, b in apart:
                other = b if a == n else a if b == n else None
                if ok and other in raw:
                    ok = all(shard(cand, g) != shard(raw[other], g) for g in gpus)
            if ok:
                break
            cand += 1
        raw[n] = cand
        cand += 1
    return raw


@dataclass
class Case:
    text: str
    rows: list                       # range_ref's form: (stream index, ts, [values])
    raw: Dict[str, int]              # label / value-key string -> raw 64-bit key
    cuts: Tuple[int, ...] = ()       # the rows are pushed in pieces cut here
    base: int = 0                    # event index of row 0
    apart: Tuple[Tuple[str, str], ...] = ()   # labels claimed to live on different shards at G = 2, 3, 4 ...
    together: bool = False           # ... and to be held together by at least one event
    value_key: Dict[int, int] = field(default_factory=dict)   # stream -> attribute of its value key
    no_stream: bool = False          # the batch goes in without a stream array (one stream)
    cap_per_row: int = 4


def _rows(pairs):
    return [(0, t, list(v)) for t, v in pairs]


def _core():
    rows = _random_rows(1200, 11)
    # 'tiny' (price<15) is first held in the second push: no such price among the first 500 rows
    rows = [(t, (s, p + 15.0 if (i < 500 and p is not None and p < 15) else p, v)) for i, (t, (s, p, v)) in enumerate(rows)]
    return Case(app(within="within 1 sec"), _rows(rows), spread(["high", "low", "tiny"], [("low", "tiny")]),
                cuts=(500,), base=7, apart=(("low", "tiny"),), together=True)


ORDER_RANGES = "price<15 as 'tiny' or price<30 as 'low'"


def _order():
    """'low' is written after 'tiny' but first seen 300 events before it; then events under 15 hold both.  Delivery of
    one event's matches is written order (tiny, low), not first-seen key order (low = 0, tiny = 1)."""
    rng = np.random.default_rng(5)
    rows = []
    for i in range(700):
        p = rng.uniform(15, 30) if i < 300 else rng.uniform(10.5, 18)
        rows.append((0, 7 * i, ["s", float(np.float32(round(p, 1))), i]))
    return Case(app(ORDER_RANGES), rows, spread(["tiny", "low"], [("tiny", "low")]), apart=(("tiny", "low"),),
                together=True)


SLICE_ROWS = (1, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 5)


@functools.lru_cache(maxsize=None)
def _edge_rows():
    return _rows(_random_rows(2 * SLICE_ROWS[-1] + 1500, 21))


def _edge_case(rows, cuts=()):
    return Case(app(within="within 1 sec"), rows, spread(["high", "low", "tiny"], [("low", "tiny")]), cuts=cuts,
                apart=(("low", "tiny"),), together=True)


@functools.lru_cache(maxsize=None)
def _edge_first():
    """the first row past 600 of the long stream whose arrival completes a match: the small push starts there, so that
    even a push of one row delivers something (matching is causal: a prefix of the stream has a prefix of its matches)"""
    t = Prepared(_edge_case(_edge_rows()[:1500])).want.trigger
    return int(t[t >= 600][0])


def _edge(n):
    """a first push that arms partial matches, then a push of n rows of the same stream of the three-range app"""
    first = _edge_first()
    return _edge_case(_edge_rows()[:first + n], cuts=(first,))


def _chunks():
    """rows for tiny chunks: a stretch that holds no range at all (null prices) and, at G = 4, a shard that never gets a
    row (three labels)"""
    rows = _random_rows(2400, 33)
    rows = [(t, (s, None if 1000 <= i < 1060 else p, v)) for i, (t, (s, p, v)) in enumerate(rows)]
    return Case(app(within="within 1 sec"), _rows(rows), spread(["high", "low", "tiny"], [("low", "tiny")]),
                apart=(("low", "tiny"),), together=True)


def _many(all_hold):
    """32 ranges: every row holds all of them (a block's 32 x 2048 copies, W = 32), or exactly one"""
    conds = [f"volume>={-k} as 'r{k}'" if all_hold else f"volume=={k} as 'r{k}'" for k in range(32)]
    rows = [(t, (s, p, i % 32 if not all_hold else i)) for i, (t, (s, p, v)) in enumerate(_random_rows(2049, 9))]
    names = [f"r{k}" for k in range(32)]
    return Case(app(" or ".join(conds), within="within 1 sec"), _rows(rows),
                spread(names, [("r0", "r1")] if all_hold else []), apart=(("r0", "r1"),) if all_hold else (),
                together=all_hold, cap_per_row=40 if all_hold else 4)


def _unread_column():
    """the conditions read `symbol`, which the query never reads"""
    return Case(app("symbol=='s1' as 'one' or symbol!='s1' as 'rest' or symbol!='s0' as 'not0'", within="within 1 sec"),
                _rows(_random_rows(900, 14)), spread(["one", "rest", "not0"], [("one", "not0")]),
                apart=(("one", "not0"),), together=True)


def _null_condition():
    """`!=` holds on a null: the rows with a null price are copies of 'ne' only"""
    rows = _random_rows(900, 15)
    rows = [(t, (s, None if i % 7 == 3 else p, v)) for i, (t, (s, p, v)) in enumerate(rows)]
    return Case(app("price!=20.5f as 'ne' or price<25 as 'lo'", cond="price>e1.price or volume>e1.volume",
                    within="within 1 sec"),
                _rows(rows), spread(["ne", "lo"], [("ne", "lo")]), apart=(("ne", "lo"),), together=True)


def _one_stream():
    c = _core()
    return Case(c.text, c.rows[:700], c.raw, apart=c.apart, together=True, no_stream=True)


SHARED = ("define stream S (price float); define stream T (v float); "
          "partition with (price>=30 as 'hi' or price<30 as 'lo' of S, v<10 as 'small' or v>=30 as 'hi' or v<30 as 'lo' "
          "of T) begin @info(name='q') from every e1=S -> e2=T[v>e1.price] select e1.price as p, e2.v as v "
          "insert into M; end;")


def _shared_label():
    """'hi' and 'lo' label ranges of both streams: one instance each; T rows under 10 hold 'small' and 'lo'"""
    rng = np.random.default_rng(8)
    rows = [(int(rng.integers(0, 2)), 3 * i, [float(np.float32(round(rng.uniform(2, 50), 1)))]) for i in range(900)]
    return Case(SHARED, rows, spread(["hi", "lo", "small"], [("small", "lo")]), apart=(("small", "lo"),), together=True)


VALUE_AND_RANGES = ("define stream S (k int); define stream T (v int); "
                    "partition with (k of S, v>0 as 'L' or v>100 as 'M' or v<0 as 'N' or v>-5 as '7' of T) begin "
                    "@info(name='q') from every e1=S -> e2=T[v>e1.k] select e1.k as k, e2.v as v insert into M; end;")


def _value_and_ranges():
    """S is keyed by value, T by ranges; the value 7 and the label '7' are one string, their raws are equal: one
    instance, the only one that sees rows of both streams"""
    rng = np.random.default_rng(12)
    rows = []
    for i in range(900):
        if rng.random() < 0.4:
            rows.append((0, 2 * i, [int(rng.choice([7, 7, 7, 5, 6]))]))
        else:
            rows.append((1, 2 * i, [int(rng.choice([3, 9, -7, 150, -2, 0, 12]))]))
    raw = spread(["L", "M", "N", "7", "5", "6"], [("L", "7"), ("M", "7")])
    return Case(VALUE_AND_RANGES, rows, raw, apart=(("L", "7"),), together=True, value_key={0: 0})


CASES = {
    "core": _core, "order": _order, "chunks": _chunks, "all32": lambda: _many(True), "one_of_32": lambda: _many(False),
    "unread_column": _unread_column, "null_condition": _null_condition, "one_stream": _one_stream,
    "shared_label": _shared_label, "value_and_ranges": _value_and_ranges,
}
for _n in SLICE_ROWS:
    for _g in (1, 2):
        CASES[f"slice{_n}x{_g}"] = functools.partial(_edge, _n * _g)
CASES["few_rows"] = functools.partial(_edge, 3)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return CASES[name]()


# ------------------------------------------------------------------------------------------- the reference
class Prepared:
    """a case's app parsed and lowered, its rows as one Batch, the reference's routing of them and the oracle's outputs
    over the routed copies.  Shared between tests (prepared() caches it); no test changes it."""

    def __init__(self, c: Case):
        self.case = c
        self.strings = {}
        self.app = C.parse(c.text)
        part = self.app.partitions[0]
        self.ctx = L.make_context(self.app, part.queries[0], part, self.strings)
        self.nfa = L.lower(self.ctx)
        self.table = L.lower_ranges(self.ctx)
        self.batch = RC.batch_of(self.app, c.rows, self.strings, base=c.base)
        self.routed = range_ref.route(self.app, c.rows, base_index=c.base, broadcast=False)
        self.want = oracle_over(self.ctx, self.batch, self.routed)
        self.label_raw = np.array([c.raw[lab] for lab in self.table.labels], np.int64)
        sids = list(self.app.streams.keys())
        attrs = [len(self.app.streams[sid].attrs) for sid in sids]
        raw = np.zeros(len(c.rows), np.int64)    # value-key rows: the raw of String.valueOf(key); range rows: ignored
        for r, (s, _, v) in enumerate(c.rows):
            if s in c.value_key:
                raw[r] = c.raw[str(v[c.value_key[s]])]
        self.raw_key = raw
        self.col_base = np.cumsum([0] + attrs)

    def held(self):
        """per input row, the labels of its copies in the reference's (written) order"""
        out = [[] for _ in self.case.rows]
        for (_, _, key, _, _), src in zip(self.routed.rows, self.routed.src):
            if key >= 0:
                out[src].append(self.routed.keys[key])
        return out


def oracle_over(ctx, b: Batch, routed: range_ref.Routed) -> Outputs:
    """the oracle engine over the reference's copies: every copy is its source row with the reference's stream, key and
    event index"""
    src = np.array(routed.src, np.int64)
    rb = Batch(len(src), 0, b.ts[src], np.array([r[1] for r in routed.rows], np.int32),
               np.array([r[2] for r in routed.rows], np.int32), [c[src] for c in b.cols],
               [None if x is None else x[src] for x in b.nulls],
               index=np.array([r[0] for r in routed.rows], np.uint64))
    eng = OracleEngine(ctx)
    eng.push(rb)
    out = eng.fetch()
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def prepared(name) -> Prepared:
    return Prepared(case(name))


def pieces(p: Prepared) -> List[Tuple[int, int]]:
    cuts = [0] + list(p.case.cuts) + [len(p.case.rows)]
    return list(zip(cuts[:-1], cuts[1:]))
