"""CPU guards of the aggregate tests: the cases themselves (enough matches, groups that repeat and continue across
pushes, and every wrong rule of agg_ref.WRONG_RULES changing some case), the front end (result types, refusals, limits)
and csrc/agg_ops.h compiled for the CPU (tests/host_agg): the scan's combine operators are associative and fold to
what the serial step gives, bit for bit."""
import ctypes as ct
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import agg_cases as A
import agg_ref as R
from parity_util import context
from siddhi_amd import lowering as L
from siddhi_amd.runtime import SiddhiAppCreationException, SiddhiAppRuntime


# ---- the cases ----------------------------------------------------------------------------------------------------
def _group_keys(case, recs):
    return [(pk if case.part else 0, tuple(R.java_string(v, t) for v, t in zip(gv, [t for _, t in case.groups])))
            for pk, gv, _ in recs]


@pytest.mark.parametrize("case", A.ALL, ids=str)
def test_case_guard(case):
    base = A.base_outputs(case)
    pushes = A.records(case, base)
    assert sum(len(p) for p in pushes) >= 200
    keys = [_group_keys(case, p) for p in pushes]
    flat = [k for p in keys for k in p]
    assert len(flat) > len(set(flat)), "no group with two matches"
    if case.cuts:    # (a one-push case has no later push; each has a three-push twin)
        seen, continued = set(), False
        for p in keys:
            continued |= bool(seen & set(p))
            seen |= set(p)
        assert continued, "no group continues in a later push"


def test_a_push_is_dropped_whole():
    case = {c.name: c for c in A.ALL}["having-drops-a-push"]
    base, rows = A.expected(case)
    assert len(base[1]) > 0 and len(rows[1]) == 0, "the second push's matches must all be dropped by having"
    assert len(rows[0]) == len(base[0]) > 0 and len(rows[2]) == len(base[2]) > 0


def test_head_null_group():
    """a group whose first arguments are all null: its sum / avg / min / max stay null while count runs"""
    case = {c.name: c for c in A.ALL}["types-DOUBLE-3push"]
    _, rows = A.expected(case)
    assert any(v[0] >= 3 and v[1] is None and v[2] is None and v[3] is None for p in rows for _, v in p)


def _flat(rows):
    return [(i, tuple("nan" if isinstance(x, float) and x != x else (R.bits(x, "DOUBLE") if isinstance(x, float) else x)
                      for x in v)) for p in rows for i, v in p]


@pytest.mark.parametrize("wrong", R.WRONG_RULES)
def test_wrong_rule_changes_a_case(wrong):
    changed = [c.name for c in A.ALL if _flat(A.expected(c, wrong)[1]) != _flat(A.expected(c)[1])]
    assert changed, f"no case tells {wrong} from the reference's rule"


# ---- the front end ------------------------------------------------------------------------------------------------
def test_result_types():
    case = A.Case("t", [(n, A.ARG[t], t) for n in ("count", "sum", "avg", "min", "max")
                        for t in ("INT", "LONG", "FLOAT", "DOUBLE")][:8])
    nfa = L.lower(context(case.agg_app()))
    assert [a[2] for a in nfa.aggs] == ["LONG"] * 4 + ["LONG", "LONG", "DOUBLE", "DOUBLE"]
    case = A.Case("t", [(n, A.ARG[t], t) for n in ("avg", "min", "max") for t in ("INT", "LONG", "FLOAT", "DOUBLE")][:8])
    nfa = L.lower(context(case.agg_app()))
    assert [a[2] for a in nfa.aggs] == ["DOUBLE"] * 4 + ["INT", "LONG", "FLOAT", "DOUBLE"]
    assert nfa.out_types == [a[2] for a in nfa.aggs]
    rt = SiddhiAppRuntime(case.agg_app(), lambda ctx: object())
    assert rt.queries[0].sel_types == nfa.out_types


def test_issue_app_lowers():
    app = """define stream S (symbol string, price float, volume int);
    partition with (symbol of S) begin
    from every e1=S[price>20] -> e2=S[price > e1.price] within 1 sec
    select e1.symbol as s, count() as n, sum(e2.volume) as vol, avg(e2.price - e1.price) as gain, max(e2.price) as hi
    group by e1.symbol having n > 3 insert into M; end;"""
    nfa = L.lower(context(app))
    assert nfa.out_types == ["STRING", "LONG", "LONG", "DOUBLE", "FLOAT"]
    assert [a and a[0] for a in nfa.aggs] == [None, 1, 2, 3, 5] and len(nfa.group_progs) == 1
    assert nfa.having_prog


def test_plain_query_lowers_as_before():
    nfa = L.lower(context(A.Case("plain", []).base_app()))
    assert nfa.aggs == [] and nfa.group_progs == [] and nfa.out_progs == []


HEAD = A.STREAM + " @info(name='q') " + A.PATTERN + " select "
REFUSED = {
    "nested": (HEAD + "sum(e2.iv) / count() as r insert into M;", "nested"),
    "nested-arg": (HEAD + "sum(count()) as r insert into M;", "nested"),
    "stdDev": (HEAD + "stdDev(e2.dv) as r insert into M;", "stdDev"),
    "distinctCount": (HEAD + "distinctCount(e2.iv) as r insert into M;", "distinctCount"),
    "and": (HEAD + "and(e2.iv > 1) as r insert into M;", "and"),
    "or": (HEAD + "or(e2.iv > 1) as r insert into M;", "or"),
    "minForever": (HEAD + "minForever(e2.iv) as r insert into M;", "minForever"),
    "maxForever": (HEAD + "maxForever(e2.iv) as r insert into M;", "maxForever"),
    "unionSet": (HEAD + "unionSet(e2.iv) as r insert into M;", "unionSet"),
    "order by": (HEAD + "count() as n order by n insert into M;", "order by"),
    "limit": (HEAD + "count() as n limit 5 insert into M;", "limit"),
    "offset": (HEAD + "count() as n offset 5 insert into M;", "offset"),
    "group by expression": (HEAD + "count() as n group by e1.iv + 1 insert into M;", "attribute references"),
    "sum of a string": (HEAD + "sum(e2.gs) as n insert into M;", "not supported for STRING"),
    "nine aggregates": (HEAD + ", ".join(f"count() as n{k}" for k in range(9)) + " insert into M;", "more than 8"),
    "five group attributes": (HEAD + "count() as n group by e1.iv, e1.lv, e1.gi, e1.gl, e1.gs insert into M;",
                              "more than 4"),
}


@pytest.mark.parametrize("engine", ["hip-front-end", "oracle"])
@pytest.mark.parametrize("what", list(REFUSED), ids=str)
def test_refused_at_creation(what, engine):
    app, word = REFUSED[what]
    if engine == "oracle":
        from oracle import OracleEngine as factory
    else:
        factory = lambda ctx: object()   # noqa: E731  (the query is lowered before the engine is made)
    with pytest.raises(SiddhiAppCreationException) as e:
        SiddhiAppRuntime(app, factory)
    assert word in str(e.value), str(e.value)


def test_limits_are_inclusive():
    L.lower(context(HEAD + ", ".join(f"count() as n{k}" for k in range(8)) + " insert into M;"))
    L.lower(context(HEAD + "count() as n group by e1.iv, e1.lv, e1.gi, e1.gl insert into M;"))


def test_oracle_refuses_aggregates():
    from oracle import OracleEngine
    with pytest.raises(SiddhiAppCreationException, match="oracle"):
        SiddhiAppRuntime(A.ALL[0].agg_app(), OracleEngine)


def test_node_pipeline_refuses_aggregates():
    from siddhi_amd import _native as N
    desc = N.build_desc(L.lower(context(A.ALL[0].agg_app())))
    with pytest.raises(SiddhiAppCreationException, match="node pipeline"):
        N.Node(desc)


# ---- agg_ops.h on the CPU -----------------------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "host_agg", "_build", "libhostagg.so")
COUNT, SUM, AVG, MIN, MAX = 1, 2, 3, 4, 5
TYPE = {"INT": 1, "LONG": 2, "FLOAT": 3, "DOUBLE": 4}


class St(ct.Structure):
    _fields_ = [("v", ct.c_int64), ("n", ct.c_int64), ("m", ct.c_uint64), ("f", ct.c_uint32), ("pad", ct.c_uint32)]

    def key(self):
        return (self.v, self.n, self.m, self.f, self.pad)


@pytest.fixture(scope="module")
def ops():
    srcs = [os.path.join(HERE, "host_agg", "harness.cpp"), os.path.join(ROOT, "siddhi_amd", "csrc", "agg_ops.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        tmp = f"{LIB}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]], check=True)
        os.replace(tmp, LIB)
    lib = ct.CDLL(LIB)
    assert lib.ha_state_bytes() == ct.sizeof(St)
    lib.ha_step.argtypes = [ct.c_int, ct.c_int, ct.POINTER(St), ct.c_int64, ct.c_int]
    lib.ha_result.argtypes = [ct.c_int, ct.c_int, ct.POINTER(St), ct.POINTER(ct.c_int)]
    lib.ha_result.restype = ct.c_int64
    lib.ha_lift.argtypes = [ct.c_int, ct.c_int, ct.c_int64, ct.c_int, ct.POINTER(St)]
    for f in (lib.ha_seed, lib.ha_unseed):
        f.argtypes = [ct.c_int, ct.c_int, ct.POINTER(St), ct.POINTER(St)]
    lib.ha_combine.argtypes = [ct.c_int, ct.c_int, ct.POINTER(St), ct.POINTER(St), ct.POINTER(St)]
    lib.ha_naive_max_combine.argtypes = [ct.c_int, ct.POINTER(St), ct.POINTER(St), ct.POINTER(St)]
    return lib


def _pool(t):
    """(bits, null) of the edge pool of a type, a null last"""
    col = {"INT": "iv", "LONG": "lv", "FLOAT": "fv", "DOUBLE": "dv"}[t]
    vals = list(A.POOLS[col])
    if t == "LONG":
        vals += [2**52, -(2**52) - 1]
    return [(R.bits(R.f32(v) if t == "FLOAT" else v, t), 0) for v in vals] + [(0, 1)]


SCANNED = [(k, t) for k in (COUNT, MIN, MAX) for t in TYPE] + [(k, t) for k in (SUM, AVG) for t in ("INT", "LONG")]


def _lift(ops, k, t, x):
    e = St()
    ops.ha_lift(k, TYPE[t], x[0], x[1], ct.byref(e))
    return e


def _comb(ops, k, t, a, b):
    o = St()
    ops.ha_combine(k, TYPE[t], ct.byref(a), ct.byref(b), ct.byref(o))
    return o


def test_scannable_pairs(ops):
    for k in (COUNT, SUM, AVG, MIN, MAX):
        for t in TYPE:
            assert bool(ops.ha_scannable(k, TYPE[t])) == ((k, t) in SCANNED)


@pytest.mark.parametrize("kind,t", SCANNED, ids=lambda x: str(x))
def test_combine_is_associative(ops, kind, t):
    pool = _pool(t)
    rng = np.random.default_rng(7)
    triples = list(itertools.product(pool, repeat=3))
    if t in ("INT", "LONG"):     # random values next to the edge pool
        lim = 2**31 if t == "INT" else 2**63
        triples += [tuple((int(rng.integers(-lim, lim)), 0) for _ in range(3)) for _ in range(300)]
    for a, b, c in triples:
        ea, eb, ec = (_lift(ops, kind, t, x) for x in (a, b, c))
        left = _comb(ops, kind, t, _comb(ops, kind, t, ea, eb), ec)
        right = _comb(ops, kind, t, ea, _comb(ops, kind, t, eb, ec))
        assert left.key() == right.key(), (a, b, c)


def _serial_and_fold(ops, kind, t, seq, combine=None, carried=0):
    """per element: (serial state key and result, folded state key and result); the first `carried` elements are the
    group's carried state, the fold starts from its seed"""
    combine = combine or (lambda a, b: _comb(ops, kind, t, a, b))
    s = St()
    for x in seq[:carried]:
        ops.ha_step(kind, TYPE[t], ct.byref(s), x[0], x[1])
    e = St()
    ops.ha_seed(kind, TYPE[t], ct.byref(s), ct.byref(e))
    out = []
    for x in seq[carried:]:
        ops.ha_step(kind, TYPE[t], ct.byref(s), x[0], x[1])
        e = combine(e, _lift(ops, kind, t, x))
        u, nl_s, nl_e = St(), ct.c_int(), ct.c_int()
        ops.ha_unseed(kind, TYPE[t], ct.byref(e), ct.byref(u))
        rs = ops.ha_result(kind, TYPE[t], ct.byref(s), ct.byref(nl_s))
        re_ = ops.ha_result(kind, TYPE[t], ct.byref(u), ct.byref(nl_e))
        out.append((s.key(), (rs, nl_s.value), u.key(), (re_, nl_e.value), bool(e.f & 8)))
    return out


def _sequences(t, count=150, length=24):
    pool = _pool(t)
    rng = np.random.default_rng(11)
    seqs = [[pool[i] for i in rng.integers(0, len(pool), length)] for _ in range(count)]
    seqs += [list(p) for p in itertools.permutations(pool[:4] + pool[-1:], 3)]
    if t in ("FLOAT", "DOUBLE"):     # NaN first / NaN later, both zeros in both orders
        z, nz, nan, one = (R.bits(v, t) for v in (0.0, -0.0, float("nan"), 1.0))
        seqs += [[(nan, 0), (one, 0), (z, 0)], [(one, 0), (nan, 0), (z, 0)], [(z, 0), (nz, 0)], [(nz, 0), (z, 0)],
                 [(0, 1), (nan, 0), (one, 0)], [(0, 1), (0, 1), (nz, 0), (z, 0), (nan, 0)]]
    return seqs


@pytest.mark.parametrize("kind,t", SCANNED, ids=lambda x: str(x))
def test_fold_equals_the_serial_step(ops, kind, t):
    inexact_seen = False
    for seq in _sequences(t):
        for carried in (0, 5):
            for s_key, s_res, u_key, u_res, inexact in _serial_and_fold(ops, kind, t, seq, carried=carried):
                if inexact:          # avg over INT / LONG past 2^53: the scan hands the run to the serial kernel
                    assert kind == AVG
                    inexact_seen = True
                    break
                assert s_res == u_res and s_key == u_key, (kind, t, seq, carried)
    if kind == AVG and t == "LONG":
        assert inexact_seen


def test_avg_inexact_flag_covers_every_inexact_sum(ops):
    """whenever the exact integer sum is not what the double additions give, the element is flagged"""
    rng = np.random.default_rng(3)
    vals = [2**52, 2**52 + 1, 2**53 - 1, 3, -5, 2**51, -(2**52) - 1, 1]
    for _ in range(300):
        seq = [(int(vals[i]), 0) for i in rng.integers(0, len(vals), 12)]
        exact, dsum = 0, 0.0
        for (s_key, s_res, u_key, u_res, inexact), x in zip(_serial_and_fold(ops, AVG, "LONG", seq), seq):
            exact += x[0]
            dsum += float(x[0])
            if float(exact) != dsum or abs(exact) >= 2**53:
                assert inexact, seq
            if not inexact:
                assert s_res == u_res


def test_a_nan_propagating_max_is_caught(ops):
    """the check above has teeth: with the IEEE-style operator in place of sg_agg_combine the fold leaves the serial
    step on a NaN that arrives later"""
    for t in ("FLOAT", "DOUBLE"):
        naive = lambda a, b: _naive(ops, t, a, b)   # noqa: E731
        bad = 0
        for seq in _sequences(t):
            for s_key, s_res, u_key, u_res, _ in _serial_and_fold(ops, MAX, t, seq, combine=naive):
                same = s_res == u_res or (s_res[1] == u_res[1] == 0 and _isnan(s_res[0], t) and _isnan(u_res[0], t))
                bad += not same
        assert bad > 0


def _naive(ops, t, a, b):
    o = St()
    ops.ha_naive_max_combine(TYPE[t], ct.byref(a), ct.byref(b), ct.byref(o))
    return o


def _isnan(b, t):
    v = R.from_bits(b, t)
    return v != v


def test_step_matches_the_python_reference(ops):
    """the serial step against agg_ref's aggregators on the edge pools (both restate the Java classes on their own)"""
    names = {COUNT: "count", SUM: "sum", AVG: "avg", MIN: "min", MAX: "max"}
    for kind, name in names.items():
        for t in TYPE:
            for seq in _sequences(t, count=40):
                ref = R._Agg(name, t, None)
                s = St()
                for bits_, null in seq:
                    ops.ha_step(kind, TYPE[t], ct.byref(s), bits_, null)
                    nl = ct.c_int()
                    got = ops.ha_result(kind, TYPE[t], ct.byref(s), ct.byref(nl))
                    want = ref.add(None if null else R.from_bits(bits_, t))
                    assert bool(nl.value) == (want is None), (name, t, seq)
                    if want is not None:
                        assert R.same_value(got, want, R.result_type(name, t)), (name, t, seq, got, want)
