"""CPU guard of the select / having cases (select_ref.py): the tables have the shape they claim, the oracle computes what
the reference restatement computes on every case, the cases hold the values that make them worth running (nulls, NaNs,
kept and dropped records, null base slots), each wrong rule a kernel could follow changes some case's answer, and programs
deeper than the device VM's stack are refused at lowering.  test_select_values.py runs the same cases on the HIP engine."""
import itertools

import numpy as np
import pytest

import select_ref as S
from oracle import OracleEngine
from parity_util import context
from siddhi_amd import lowering as L
from siddhi_amd.runtime import SiddhiAppCreationException, SiddhiManager


# ------------------------------------------------------------------------------------------- table shape
def test_every_ordered_pool_pair_appears_once():
    pairs = list(zip(S.SEQ, S.SEQ[1:]))
    assert len(S.SEQ) == 577 and len(pairs) == len(set(pairs)) == S.NPOOL ** 2
    assert set(pairs) == set(itertools.product(range(S.NPOOL), repeat=2))
    # ... and the engine's matches are those pairs: the plain twin's base values, record by record
    for name in ("pairs-INT-search", "pairs-INT-tiled", "pairs-INT-once"):
        case = S.BY_NAME[name]
        want = [(S.POOLS["INT"][i], S.POOLS["INT"][j]) for i, j in pairs]
        assert [(v[("e1", "a")], v[("e2", "a")]) for v in S.base_values(case)] == want, name


def test_every_operator_and_type_pair_is_in_some_group():
    seen = {(e[0], S.etype(e[1]), S.etype(e[2])) for g in S.GROUPS.values() for e in g
            if e[1][0] == "var" and e[2][0] == "var"}
    assert seen >= set(itertools.product(S.MATH_OPS, S.TYPES, S.TYPES))
    constants = {(side, c[1]) for e in S.CONSTANTS for side in (1, 2) for c in [e[side]] if c[0] == "const"}
    assert constants == set(itertools.product((1, 2), S.TYPES))          # a constant of each type on either side
    assert any(S.etype(e[1]) != S.etype(e) for e in S.NESTED if e[1][0] in S.MATH_OPS)


def test_no_query_has_more_than_32_outputs():
    for case in S.ALL:
        assert len(case.exprs) <= 32 and len(case.base) <= 32, case.name
    nfa = L.lower(context(S.WIDE.app()))
    assert (len(nfa.out_progs), len(nfa.select), len(nfa.retained)) == (32, 32, 16)


def test_pools_hold_the_named_values():
    for t in S.TYPES:
        assert len(S.POOLS[t]) == S.NPOOL and S.POOLS[t].count(None) == 1, t
    P = {t: [x for x in p if x is not None] for t, p in S.POOLS.items()}
    assert set(P["INT"]) >= {0, 1, -1, 7, -7, 3, 13, 2**24 - 1, 2**24, 2**24 + 1, -2**31, -2**31 + 1, 2**31 - 1, 2**31 - 2,
                             46341, -46341, 65536}
    assert set(P["LONG"]) >= {0, 1, -1, 7, -7, 3, 13, 2**24 + 1, 2**53 + 1, -2**53 - 1, -2**63, -2**63 + 1, 2**63 - 1,
                              2**63 - 2, 2**60 + 2**36 + 1, 2**40 + 2**16 + 1, 3037000500, -3037000500, 2**31, 2**32, 2**62}
    f32, f64 = np.finfo(np.float32), np.finfo(np.float64)
    for t, fi, more in (("FLOAT", f32, [float(np.float32(0.1)), 2.0**24 - 1, 2.0**24, 2.0**24 + 2, 2.0**53,
                                         float(np.float32(1e20)), float(np.float32(1e-20))]),
                        ("DOUBLE", f64, [0.1, 16777217.0, 2.0**53, 2.0**53 + 2, 1e20, 1e-20, 1e200, 1e-200])):
        vals = P[t]
        assert any(x != x for x in vals), t
        rest = [x for x in vals if x == x]
        assert set(rest) >= {1.0, -1.0, -2.5, 7.25, 3.0, float(fi.max), -float(fi.max), float(fi.tiny), np.inf, -np.inf,
                             *more}, t
        assert sorted(np.signbit(x) for x in rest if x == 0) == [False, True], t       # 0.0 and -0.0
        den = float(fi.smallest_subnormal)
        assert den in rest and -den in rest, t
        assert all(float(np.array(x, S.NP[t])) == x for x in rest), t                  # every member is a value of its type


def test_the_long_that_rounds_twice_through_a_double():
    b = 2**60 + 2**36 + 1
    assert S.to_bits(S._jmath("+", b, 0.0, "FLOAT"), "FLOAT") == 0x5d800001             # Long.floatValue()
    assert S.to_bits(S._jmath("+", b, 0.0, "FLOAT", {"long_to_float_through_double"}), "FLOAT") == 0x5d800000
    assert b in S.POOLS["LONG"]


# ------------------------------------------------------------------------------------------- oracle == reference
def _distinct(cases):
    """one case per (query text, rows): the sweep's routes share both"""
    seen, out = set(), []
    for c in cases:
        k = (c.app(), c.rows, str(c.arg if not isinstance(c.arg, np.ndarray) else c.arg.tobytes()), tuple(c.cuts))
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _distinct(S.ALL), ids=str)
def test_oracle_equals_reference(case):
    """values under the comparison helper; trigger / ts / key / group exactly those of the plain twin's kept records.
    The pair groups are the 46,080-result sweep (24 x 24 ordered pairs, 16 type pairs, 5 operators)."""
    assert len(S._plain(case.name)) >= case.floor
    S.check(case, S.oracle(case), "oracle")


# ------------------------------------------------------------------------------------------- conditions on the cases
def _always_null(e):
    return e[0] in "/%" and e[2][0] == "const" and e[2][2] == 0


def _nan_possible(e):
    return S.etype(e) in ("FLOAT", "DOUBLE") and any(S.COLTYPE[v[2]] in ("FLOAT", "DOUBLE") for v in S.leaves(e))


@pytest.mark.parametrize("group", list(S.GROUPS))
def test_group_columns_have_nulls_values_and_nans(group):
    """every arithmetic output column has null and non-null results, at most half of them null, and NaN results where a
    FLOAT / DOUBLE attribute feeds it (an INT attribute and a constant cannot make one); a zero constant divisor makes
    the whole column null, which is its point"""
    for name in (f"{group}-search", f"{group}-once"):
        case = S.BY_NAME[name]
        _, vals, null = S.expected(name)
        assert len(vals) == S.NPOOL ** 2
        for k, e in enumerate(case.exprs):
            n_null = int(null[:, k].sum())
            if _always_null(e):
                assert n_null == len(vals), (name, S.text(e))
                continue
            assert 0 < n_null <= len(vals) // 2, (name, S.text(e), n_null)
            nan = S.is_nan_bits(vals[:, k], S.etype(e)) & ~null[:, k]
            assert nan.any() == _nan_possible(e), (name, S.text(e))
            assert (~nan & ~null[:, k]).any(), (name, S.text(e))


def test_sweep_creates_nans_and_denormals():
    """inf - inf, 0 * inf, inf % x; a denormal result; a long operand that needs more than 53 bits"""
    case = S.BY_NAME["pairs-FLOAT-search"]
    _, vals, null = S.expected(case.name)
    base = S.base_values(case)
    for op, pick in (("-", lambda x, y: x == y == np.inf), ("*", lambda x, y: x == 0 and y == np.inf),
                     ("%", lambda x, y: x == np.inf and y == 3.0)):
        k = case.exprs.index((op, S.E1["f"], S.E2["f"]))
        rows = [r for r, v in enumerate(base) if None not in (v[("e1", "f")], v[("e2", "f")])
                and pick(v[("e1", "f")], v[("e2", "f")])]
        assert rows and all(S.is_nan_bits(vals[rows, k], "FLOAT")), op
    k = case.exprs.index(("*", S.E1["f"], S.E2["f"]))
    tiny = float(np.finfo(np.float32).tiny)
    got = np.abs((vals[:, k] & 0xFFFFFFFF).astype(np.uint32).view(np.float32)[~null[:, k]])
    assert ((got > 0) & (got < tiny)).any()


@pytest.mark.parametrize("case", S.HAVING_CASES, ids=str)
def test_having_cases_keep_some_and_drop_some(case):
    assert 0 < len(S.expected(case.name)[1]) < len(S._plain(case.name))


def test_compaction_cases_keep_what_their_names_say():
    for case in S.COMPACT_CASES:
        kept = S.expected(case.name)[1]
        flags = case.arg
        assert len(S._plain(case.name)) == len(flags) and len(kept) == int(flags.sum()), case.name
        assert kept[:, 0].tolist() == np.flatnonzero(flags).tolist(), case.name          # e1.id of the kept records
    two = S.BY_NAME["compact-two_pushes-some_then_none"].arg
    assert two[:300].any() and not two[300:].any()


def test_wide_case_sets_and_clears_bit_31():
    _, vals, null = S.expected(S.WIDE.name)
    assert 0 < null[:, 31].sum() < len(null)
    o = S._plain(S.WIDE.name)                      # ... and so does base slot 31 of the records the select pass reads
    assert 0 < o.vnull[:, 31].sum() < len(o)


@pytest.mark.parametrize("case", S.GROUP_CASES + S.ROUTE_CASES, ids=str)
def test_twin_cases_have_matches_and_null_base_slots(case):
    o = S._plain(case.name)
    assert len(o) >= max(case.floor, 200)
    assert o.vnull.any()
    if case.name == "sequence_lanes":       # `e3 or e4`: the side that did not match is a null base slot
        base = case.base
        for ref in ("e3", "e4"):
            k = [i for i, v in enumerate(base) if v[1] == ref]
            assert o.vnull[:, k].all(axis=1).any() and not o.vnull[:, k].all(axis=1).all(), ref


def test_depth_cases_wrap_and_filter():
    sel, hav, fil = S.DEPTH_CASES
    _, vals, null = S.expected(sel.name)
    exact = [sum(v[(("e1", "e2")[j % 2], "a")] for j in range(S.VM_DEPTH)) for v in S.base_values(sel)
             if None not in v.values()]
    assert any(abs(x) >= 2**31 for x in exact)                      # some sums wrap
    assert 0 < len(S.expected(hav.name)[1]) < len(S._plain(hav.name))
    assert 200 <= len(S._plain(fil.name)) < S.N_SWEEP - 1


# ------------------------------------------------------------------------------------------- sensitivity
WRONG = {
    "long_to_float_through_double": "pairs-LONG-search",
    "floor_division": "pairs-INT-search",
    "remainder_signed_by_divisor": "pairs-INT-search",
    "min_by_minus_one_saturates": "pairs-LONG-search",
    "float_arithmetic_in_double": "pairs-LONG-search",
    "zero_divisor_divides": "pairs-FLOAT-search",
    "nan_divisor_is_null": "pairs-FLOAT-search",
    "float_long_equal_in_float": "having-long==float",
    "long_float_order_in_double": "having-long>float",
    "null_not_equal_is_false": "having-null-!=",
}


@pytest.mark.parametrize("rule", S.WRONG_RULES)
def test_each_wrong_rule_changes_an_answer(rule):
    """an engine that followed `rule` instead of the reference's would fail the named case"""
    case = S.BY_NAME[WRONG[rule]]
    where, vals, null = S.reference(case, frozenset({rule}))
    right = S.expected(case.name)
    got = S.Outputs(where.trigger, where.ts, where.key, where.group, vals, null)
    with pytest.raises(AssertionError):
        S.check(case, got, rule)
    ok = S.Outputs(*[getattr(right[0], f) for f in ("trigger", "ts", "key", "group")], right[1], right[2])
    S.check(case, ok, "the reference itself")


# ------------------------------------------------------------------------------------------- depth of the VM programs
def _programs(case):
    nfa = L.lower(context(case.app()))
    return {"select": nfa.out_progs[0], "having": nfa.having_prog, "filter": nfa.states[1].prog}


def test_depth_16_lowers():
    assert L.VM_STACK == S.VM_DEPTH == 16
    for case, clause in zip(S.DEPTH_CASES, ("select", "having", "filter")):
        assert L.prog_depth(_programs(case)[clause]) == 16, case.name


@pytest.mark.parametrize("clause,word", [("select", "select attribute x0"), ("having", "having"),
                                         ("filter", "filter of state 1 (e2)")])
def test_depth_17_is_refused(clause, word, monkeypatch):
    case = {c.name.split("-")[1]: c for c in S.depth_cases(17)}[clause]
    with pytest.raises(L.LoweringError, match=word.replace("(", r"\(").replace(")", r"\)")):
        L.lower(context(case.app()))
    with pytest.raises((SiddhiAppCreationException, L.LoweringError)):
        SiddhiManager(engine=OracleEngine).createSiddhiAppRuntime(case.app())
    monkeypatch.setattr(L, "VM_STACK", 64)          # (the limit is the only thing in the way)
    assert L.prog_depth(_programs(case)[clause]) == 17


def test_forty_operands_are_refused():
    case = S.sweep_case("depth40", [S.int_sum(40)])
    with pytest.raises(L.LoweringError, match="stack of 40"):
        L.lower(context(case.app()))
