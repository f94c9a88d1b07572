"""The guard of value_cases.py, on the CPU: every case lowers to the shape it is meant for, the oracle delivers exactly
the matches of the row-at-a-time reference (closed_form_ref.py, which shares no code with the lowering, the oracle or
the kernels), and the case has enough matches to mean something.  Then, per value type, the reference is run again with
one deliberately wrong compare after another, and each must change the match list of at least one case of that type:
a kernel that compared that way could not pass test_closed_form_values.py / test_pred_pass.py."""
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))

import range_ref  # noqa: E402
import value_cases as V  # noqa: E402
from oracle import OracleEngine  # noqa: E402  (checker engine; CPU)
from parity_util import run_engine  # noqa: E402
from siddhi_amd import lowering as L  # noqa: E402

exact = range_ref._compare
_ORACLE = {}


def oracle_triples(case):
    if case.name not in _ORACLE:
        _ORACLE[case.name] = V.triples(run_engine(OracleEngine, case.app, V.pushes(case)))
    return _ORACLE[case.name]


def check_case(case):
    nfa = L.lower(V._context(case.app))
    if case.kind == "every":
        assert nfa.shape == L.SHAPE_EVERY_NEXT_CMP
    elif case.kind == "once":
        assert nfa.shape == L.SHAPE_NEXT_CMP_ONCE
    else:
        assert nfa.shape == L.SHAPE_GENERAL and nfa.states[0].local and nfa.states[0].prog
    want = V.reference(case)
    assert oracle_triples(case) == want
    assert len(want) >= case.floor, len(want)
    return want


@pytest.mark.parametrize("case", V.CLOSED, ids=str)
def test_closed_form_case(case):
    check_case(case)


@pytest.mark.parametrize("nulls", [True, False], ids=["nulls", "no_nulls"])
@pytest.mark.parametrize("case", V.PRED + V.DEPTH, ids=str)
def test_predicate_case(case, nulls):
    check_case(case if nulls else V.without_nulls(case))


def test_every_constant_passes_some_rows_and_fails_some():
    """a predicate case may match nothing by design (`v == 16777217L` on a FLOAT column); over the six operators every
    (column, constant) passes some rows and fails others"""
    for typ, consts in V.CONSTANTS.items():
        for c in consts:
            counts = [len(V.reference(V.BY_NAME[f"P1-{typ}-{V._cname(c)}-{op}"])) for op in V.OPS6]
            assert 0 < max(counts) and min(counts) < V.PRED_N - 1, (typ, c, counts)
            assert counts[0] + counts[1] == V.PRED_N - 1, (typ, c, counts)       # == and != part the rows
    assert len(V.reference(V.BY_NAME["P1-FLOAT-16777217L-=="])) == 0             # double domain: 2^24 != 2^24 + 1
    assert len(V.reference(V.BY_NAME["P1-FLOAT-16777217->="])) > len(V.reference(V.BY_NAME["P1-FLOAT-16777217->"]))
    case = V.BY_NAME["P1-INT-16777216p0f-=="]                                    # f32 domain: 2^24 + 1 compares equal
    b = V.batch(case)
    near = np.isin(b.cols[2], [2**24, 2**24 + 1]) & (b.nulls[2] == 0)
    assert (b.cols[2][near] == 2**24 + 1).any()
    assert [e1 for _, e1, _ in V.reference(case)] == np.flatnonzero(near[:-1]).tolist()


def test_depth_cases_hit_every_register_stack():
    for case, (lo, hi) in zip(V.DEPTH, V.DEPTH_BUCKETS):
        d = L.prog_depth(L.lower(V._context(case.app)).states[0].prog)
        assert lo < d <= hi, (case.name, d)
        n = len(V.reference(case))
        assert V.PRED_N // 20 < n < V.PRED_N - V.PRED_N // 20, (case.name, n)


# ------------------------------------------------------------------------------------------- wrong compares
def _bits(t, v):
    return struct.unpack("<i", struct.pack("<f", v))[0] if t == "FLOAT" else struct.unpack("<q", struct.pack("<d", v))[0]


def _to_f32(v):
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def long_as_double(op, lt, lv, rt, rv):
    if lt == rt == "LONG" and lv is not None and rv is not None:
        return exact(op, "DOUBLE", float(lv), "DOUBLE", float(rv))
    return exact(op, lt, lv, rt, rv)


def int_as_float32(op, lt, lv, rt, rv):
    if lt == rt == "INT" and lv is not None and rv is not None:
        return exact(op, "FLOAT", range_ref.int_to_f32(lv), "FLOAT", range_ref.int_to_f32(rv))
    return exact(op, lt, lv, rt, rv)


def double_as_float32(op, lt, lv, rt, rv):
    if lt == rt == "DOUBLE" and lv is not None and rv is not None:
        return exact(op, "FLOAT", _to_f32(lv), "FLOAT", _to_f32(rv))
    return exact(op, lt, lv, rt, rv)


def bit_patterns(op, lt, lv, rt, rv):
    if lt == rt and lt in ("FLOAT", "DOUBLE") and lv is not None and rv is not None:
        return exact(op, "LONG", _bits(lt, lv), "LONG", _bits(rt, rv))
    return exact(op, lt, lv, rt, rv)


def nan_on_top(op, lt, lv, rt, rv):
    if lt == rt and lt in ("FLOAT", "DOUBLE") and lv is not None and rv is not None:
        ln, rn = math.isnan(lv), math.isnan(rv)
        if ln or rn:
            return exact(op, "INT", int(ln), "INT", int(rn))
    return exact(op, lt, lv, rt, rv)


def null_as_zero(op, lt, lv, rt, rv):
    zero = lambda t: 0 if t in ("INT", "LONG") else 0.0
    return exact(op, lt, zero(lt) if lv is None else lv, rt, zero(rt) if rv is None else rv)


def swap(x, y):
    def compare(op, lt, lv, rt, rv):
        return exact({x: y, y: x}.get(op, op), lt, lv, rt, rv)
    compare.__name__ = f"swap_{x}_{y}"
    return compare


def constant_as_column_type(op, lt, lv, rt, rv):
    """`v OP c` with c converted to v's type (v the left operand) where the exact compare converts both to the domain"""
    if lt != rt and lv is not None and rv is not None:
        if lt == "INT":
            rv = max(-2**31, min(2**31 - 1, int(rv)))        # (int) of a long / float / double, saturating
        else:
            rv = range_ref.int_to_f32(rv) if rt in ("INT", "LONG") else _to_f32(rv)
        rt = lt
    return exact(op, lt, lv, rt, rv)


VALUE_WRONGS = {
    "INT": [int_as_float32],
    "LONG": [long_as_double],
    "FLOAT": [bit_patterns, nan_on_top],
    "DOUBLE": [double_as_float32, bit_patterns, nan_on_top],
}
EVERY_TYPE = [null_as_zero, swap(">", ">="), swap("<", "<=")]
WRONGS = [(typ, w) for typ in V.TYPES for w in VALUE_WRONGS[typ] + EVERY_TYPE]


def defeated_by(cases, **kw):
    """the first case whose match list the wrong rule changes"""
    for case in cases:
        if V.reference(case, **kw) != V.reference(case):
            return case.name
    return None


@pytest.mark.parametrize("typ,wrong", WRONGS, ids=[f"{t}-{w.__name__}" for t, w in WRONGS])
def test_wrong_compare_is_defeated(typ, wrong):
    assert defeated_by([c for c in V.CLOSED if c.typ == typ], compare=wrong) is not None


@pytest.mark.parametrize("typ", V.TYPES)
@pytest.mark.parametrize("kind", ["every", "once"])
def test_wrong_expiry_is_defeated(typ, kind):
    """`>= within` in place of `> within`: same-key rows exactly `within` apart exist in every case"""
    cases = [c for c in V.CLOSED if c.typ == typ and c.kind == kind]
    assert defeated_by(cases, expired=lambda dt, within: dt >= within) is not None


def null_fails_not_equal(op, lt, lv, rt, rv):
    """a null operand makes every compare false, `!=` included (it is true: NotEqualCompareConditionExpressionExecutor)"""
    return False if lv is None or rv is None else exact(op, lt, lv, rt, rv)


@pytest.mark.parametrize("typ,family", [("INT", "P1"), ("FLOAT", "P1"), ("FLOAT", "P4")])
def test_null_failing_not_equal_is_defeated(typ, family):
    """P1 observes the filter's bits row by row; in P4 (the once route) a null price binds e1 and holds its key for good"""
    cases = [c for c in V.PRED if c.typ == typ and c.name.startswith(family) and c.op == "!="]
    assert cases
    for case in cases:
        assert V.reference(case, compare=null_fails_not_equal) != V.reference(case), case.name


@pytest.mark.parametrize("typ,family", [("INT", "P1"), ("INT", "P2"), ("FLOAT", "P1"), ("FLOAT", "P2"), ("FLOAT", "P3"),
                                        ("FLOAT", "P4")])
def test_constant_in_the_column_type_is_defeated(typ, family):
    cases = [c for c in V.PRED if c.typ == typ and c.name.startswith(family)]
    assert defeated_by(cases, compare=constant_as_column_type) is not None


def test_reference_restates_the_rule_by_hand():
    """five rows of one key, `every e1=S[w >= 100] -> e2=S[v > e1.v] within 1 sec`: row 1 completes row 0 exactly 1000 ms
    later, row 3 comes 1001 ms after row 2 (dropped), a null never completes and is never completed"""
    case = V.BY_NAME["tiled-INT->-stack"]
    every, a, b, op, within = V.pattern(case)
    assert (every, op, within, a.attr, b.attr) == (True, ">", 1000, 2, 2)
    rows = [(0, t, 0, [i, 0, v, w]) for i, (t, v, w) in enumerate(
        [(0, 30, 500), (1000, 31, 500), (5000, 25, 500), (6001, 35, 500), (6500, None, 500), (7001, 36, 99)])]
    import closed_form_ref as R
    assert R.every_next(rows, a, b, op, within, True) == [(1, 0, 1), (5, 3, 5)]
    assert R.once(rows, a, b, op, within, True) == [(1, 0, 1)]
    assert R.once(rows[2:], a, b, op, within, True) == []          # row 3 expires the partial: the key is done
