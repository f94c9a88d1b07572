"""Range routing against a row-at-a-time reference (range_ref.py) that shares no code with the routers.

The host router (runtime._range_mask / _range_route / _broadcast) and the postfix programs of lowering.lower_ranges
(through the numpy interpreter of test_range_router.py) are compared with range_ref.route over one all-type stream:
every ordered pair of numeric columns x the six operators, every numeric column against the edge constants, STRING and
BOOL equality, `is null` of every type and the nested forms, on rows drawn from edge pools (NaN, signed zeros and
infinities, 2^24 +- 1, 2^53 +- 1, 2^60 + 2^36 + 1, 2^63, the integer extremes) with nulls.  Two host bugs the
reference showed are pinned with their fixes: `is null` of a non-BOOL attribute was refused in a range condition, and
a flush holding rows of a value-partitioned, a range-partitioned and an unpartitioned stream handed out the value keys'
ids before the labels', so an unpartitioned row reached instances that later rows created."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))

import range_cases as RC  # noqa: E402
import range_ref  # noqa: E402
from oracle import OracleEngine  # noqa: E402  (checker engine; CPU)
from siddhi_amd import SiddhiManager  # noqa: E402
from siddhi_amd import compiler as C  # noqa: E402
from siddhi_amd import lowering as L  # noqa: E402
from test_range_partition import app as price_app  # noqa: E402
from test_range_router import CONDITIONS, interpret  # noqa: E402

from range_cases import IS_NULL, MIXED, MIXED3, TYPED_APPS, check_flush_granularity  # noqa: E402
from range_cases import mixed_rows, price_rows, typed_case  # noqa: E402


# ------------------------------------------------------------------------------------------- the reference itself
def test_reference_rounds_a_long_to_binary32_once():
    v = 2**60 + 2**36 + 1           # one rounding: 2^60 + 2^37; through a double (2^60 + 2^36, a tie): 2^60
    assert v in RC.POOLS["LONG"] and range_ref.int_to_f32(v) == 2**60 + 2**37 != float(np.float32(float(v)))
    for x in RC.POOLS["LONG"] + RC.POOLS["INT"]:
        assert range_ref.int_to_f32(x) == float(np.float32(np.int64(x))), x


def test_reference_compare_domains_by_hand():
    d = C.StreamDefinition("S", [("l", "LONG"), ("f", "FLOAT"), ("i", "INT"), ("d", "DOUBLE")])

    def h(text, l=None, f=None, i=None, dd=None):
        a = C.parse(f"define stream S (l long, f float, i int, d double); partition with ({text} as 'x' of S) "
                    "begin from every e1=S -> e2=S select e1.i as i insert into M; end;")
        return range_ref.holds(a.partitions[0].ranges["S"][0][0], d, [l, f, i, dd])
    big = 16777217                                       # (float) 16777217 = 16777216.0f
    assert not h("l==f", big, 16777216.0) and h("l!=f", big, 16777216.0)       # == / != as double
    assert h("l>=f", big, 16777216.0) and not h("l>f", big, 16777216.0)        # > >= < <= as float
    assert h("i==f", None, 16777216.0, big) and not h("i==d", i=big, dd=16777216.0)
    assert h("l==d", 2**53 + 1, dd=2.0**53) and not h("l==9007199254740992l", 2**53 + 1)
    assert not h("l>f", None, 1.0) and h("l!=f", None, 1.0) and not h("f==f", f=float("nan"))
    assert h("l is null") and h("not (l>1l)") and not h("not (l is null) and i>0", 1, i=0)


# ------------------------------------------------------------------------------------------- typed apps
def test_typed_apps_cover_the_condition_matrix():
    conds = [c for _, part in TYPED_APPS for c in part]
    assert len(conds) == len(set(conds)) and all(len(part) <= 32 for _, part in TYPED_APPS)
    assert len(RC.pair_conditions()) == 8 * 7 * 6 and set(RC.pair_conditions()) <= set(conds)
    assert len(RC.NUMERIC_COLS) == 8
    for col in RC.NUMERIC_COLS:
        for k in RC.CONSTANTS:
            assert {f"{col}{op}{k}" for op in RC.OPS} <= set(conds)
    assert set(CONDITIONS) <= set(conds)              # every condition of test_range_router.py, nested forms included


@pytest.mark.parametrize("k", range(len(TYPED_APPS)))
def test_every_condition_holds_somewhere_and_fails_somewhere(k):
    case = typed_case(k)
    held = Counter(case.want.keys[r[2]] for r in case.want.rows)
    for j, cond in enumerate(case.conds):
        if cond in RC.CONSTANT_BY_DESIGN:
            assert held[f"r{j}"] == (case.n if RC.CONSTANT_BY_DESIGN[cond] else 0), cond
        else:
            assert 0 < held[f"r{j}"] < case.n, (cond, held[f"r{j}"])


def test_constant_conditions_are_the_named_ones():
    assert set(RC.CONSTANT_BY_DESIGN) <= {c for _, part in TYPED_APPS for c in part}


@pytest.mark.parametrize("k", range(len(TYPED_APPS)))
def test_host_router_equals_reference(k):
    case = typed_case(k)
    rt, b = case.runtime()
    got = rt._route_ranges(0, rt.queries[0], b, b.stream)
    assert list(rt.key_dicts[0]) == case.want.keys            # the same labels, created in the same order
    RC.assert_routed(got, case.want, b, rt.app, rt.strings)
    rt.shutdown()


@pytest.mark.parametrize("k", range(len(TYPED_APPS)))
def test_lowered_programs_equal_reference(k):
    case = typed_case(k)
    rt, b = case.runtime()
    table = L.lower_ranges(rt.queries[0].ctx)
    want = case.masks()
    assert len(table.ranges) == len(case.conds)
    for j, (s, lab, prog) in enumerate(table.ranges):
        assert (s, table.labels[lab]) == (0, f"r{j}")
        got = interpret(prog, b.cols, b.nulls, case.n)
        assert np.array_equal(got, want[j]), case.conds[j]
    rt.shutdown()


# ------------------------------------------------------------------------------------------- `is null` of any type
@pytest.mark.parametrize("ranges", IS_NULL)
def test_is_null_of_a_non_bool_attribute_routes_as_the_reference(ranges):
    """lowering._check_range_cond took the operand of `is null` for a condition and refused every attribute that is
    not BOOL ("range partition condition must be a boolean expression")"""
    text = price_app(ranges)
    rt = SiddhiManager(engine=OracleEngine).createSiddhiAppRuntime(text)
    rows = price_rows(300, 4)
    want = range_ref.route(C.parse(text), rows, base_index=10)
    assert len(want.keys) == ranges.count(" as ") and 0 < len(want.rows)
    b = RC.batch_of(rt.app, rows, rt.strings, base=10)
    got = rt._route_ranges(0, rt.queries[0], b, b.stream)
    assert list(rt.key_dicts[0]) == want.keys
    RC.assert_routed(got, want, b, rt.app, rt.strings)
    table = L.lower_ranges(rt.queries[0].ctx)
    for s, lab, prog in table.ranges:
        rows_of = sorted({src for r, src in zip(want.rows, want.src) if want.keys[r[2]] == table.labels[lab]})
        assert np.flatnonzero(interpret(prog, b.cols, b.nulls, b.n)).tolist() == rows_of
    rt.shutdown()


def test_is_null_operand_must_be_an_attribute_of_the_stream():
    from siddhi_amd import SiddhiAppCreationException
    for ranges in ("nope is null as 'x'", "price as 'x'"):
        with pytest.raises(SiddhiAppCreationException):
            SiddhiManager(engine=OracleEngine).createSiddhiAppRuntime(price_app(ranges))


# ------------------------------------------------------------------------------------------- flush granularity
def test_three_row_mixed_flush_delivers_nothing_however_it_is_flushed():
    """T(1) creates 'L'; G(7) reaches the instances that exist, 'L' alone; S(5) creates '5', which never saw G.  In
    one flush the value key 5 used to take id 0 ahead of 'L', and G's copies went to ids 0 and 1: [(7, 5, None)]."""
    rows = [(1, 0, [1]), (2, 1, [7]), (0, 2, [5])]
    assert check_flush_granularity(OracleEngine, MIXED3, rows) == []
    assert range_ref.route(C.parse(MIXED3), rows).keys == ["L", "5"]


def late_instances(text, rows):
    """(value keys, labels) created after the first row of the unpartitioned stream G"""
    want = range_ref.route(C.parse(text), rows)
    first_g = min(r for r, (s, _, _) in enumerate(rows) if s == 2)
    made = {}
    for (_, s, key, _, _), src in zip(want.rows, want.src):
        if s in (0, 1) and key not in made:
            made[key] = (src, s)
    assert sorted(made) == list(range(len(want.keys)))
    late = [s for src, s in made.values() if src > first_g]
    return late.count(0), late.count(1)


def test_mixed_flush_random_interleaving():
    rows = mixed_rows(200, 6)
    nv, nl = late_instances(MIXED, rows)
    assert nv >= 3 and nl >= 2
    check_flush_granularity(OracleEngine, MIXED, rows, min_delivered=20)
