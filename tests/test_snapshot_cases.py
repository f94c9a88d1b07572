"""The guard of snapshot_cases.py, on the CPU: every case lowers to the shape or lane rule it is meant for, the oracle
delivers enough matches over the whole stream, every cut is one that state has to cross (an oracle match straddles it),
the decoy stream really is another stream, and an engine that forgets everything at a cut -- the oracle run piece by
piece with a fresh engine per piece -- gives another output than the uninterrupted run.  test_snapshot_cuts.py runs the
same cases on the GPU; it cannot quietly degrade while these hold."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))

import snapshot_cases as S  # noqa: E402
from parity_util import context  # noqa: E402
from siddhi_amd import _native as N  # noqa: E402
from siddhi_amd import lowering as L  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "host_interp"))
from host_engine import _load  # noqa: E402


def _desc(case):
    return N.build_desc(L.lower(context(case.app)))


def seq_small(nfa) -> bool:
    """seq.h sg_seq_small over the lowered states: at most 4 states, 6 count-chain entries and 3 elements (the second
    member of a logical pair is no element of its own), so a pool of elements + 1 <= 4 partials"""
    chain = sum(s.max_count for s in nfa.states if s.kind == L.K_COUNT)
    elements = sum(1 for i, s in enumerate(nfa.states) if not (s.kind == L.K_LOGICAL and 0 <= s.partner < i))
    return len(nfa.states) <= 4 and chain <= 6 and elements + 1 <= 4


@pytest.mark.parametrize("case", S.CASES, ids=str)
def test_case_takes_its_route(case):
    nfa = L.lower(context(case.app))
    lib = _load()
    if case.family == "every":
        assert nfa.shape == L.SHAPE_EVERY_NEXT_CMP and not case.engine.get("force_general")
    elif case.family == "once":
        assert nfa.shape == L.SHAPE_NEXT_CMP_ONCE
    elif case.family == "absent":
        assert nfa.shape == L.SHAPE_EVERY_ABSENT_EQ and not case.engine.get("force_general")
    elif case.family == "machine":
        # the arena route: forced past the closed form, and past the lanes where a lane rule would take the query
        assert case.engine.get("force_general") or nfa.shape == L.SHAPE_GENERAL
        lanes = lib.hi_pp_rule(ct.byref(_desc(case))) or lib.hi_seq_rule(ct.byref(_desc(case)))
        assert (case.engine.get("partial_lanes") == -1) == bool(lanes), lanes
    elif case.family == "lanes":
        assert lib.hi_pp_rule(ct.byref(_desc(case))) == 1 and case.engine.get("force_general")
        assert case.engine.get("partial_lanes", 0) >= 0
    else:
        assert case.family == "seq"
        assert lib.hi_seq_rule(ct.byref(_desc(case))) == 1 and lib.hi_pp_rule(ct.byref(_desc(case))) == 0
        assert nfa.shape == L.SHAPE_GENERAL and not case.engine
        assert seq_small(nfa) == case.seq_small


def test_cases_cover_what_they_are_meant_to():
    fam = lambda f: [c for c in S.CASES if c.family == f]   # noqa: E731
    every = fam("every")
    for typ in ("INT", "LONG", "FLOAT", "DOUBLE"):
        routes = {c.source.route for c in every if c.source.typ == typ}
        assert "carry" in routes and len(routes) >= 3, (typ, routes)
        modes = {c.name.rsplit("-", 1)[1] for c in every if c.source.typ == typ and c.source.route == "carry"}
        assert modes == {"stack", "list"}, (typ, modes)
    for route in ("search", "flat_walker", "sorted", "redo", "wide", "time_back", "two_streams"):
        assert len({c.source.typ for c in every if c.source.route == route}) >= 2, route
    assert any(c.source.engine.get("ring_cap") == 2 for c in every)
    assert sorted(c.source.typ for c in fam("once")) == ["DOUBLE", "FLOAT", "INT", "LONG"]
    assert {c.shape for c in fam("lanes")} >= set(S.SHAPES) and {c.shape for c in fam("seq")} >= set(S.SEQ_SHAPES)
    assert {c.seq_small for c in fam("seq")} == {True, False}          # both SeqState layouts
    assert {c.family for c in S.CASES} == {"every", "once", "absent", "machine", "lanes", "seq"}
    assert {S.BY_NAME[n].family for n in S.BLOB_CASES} == {"every", "once", "absent", "machine", "lanes", "seq"}
    assert {S.BY_NAME[n].seq_small for n in S.BLOB_CASES} >= {True, False}


@pytest.mark.parametrize("case", S.CASES, ids=str)
def test_every_cut_carries_state(case):
    b, want, cuts = S.whole(case), S.want(case), S.cuts(case)
    assert len(want) >= case.floor > 0, (len(want), case.floor)
    assert len(cuts) >= 12 and cuts == sorted(set(cuts)) and 0 < cuts[0] and cuts[-1] < b.n, cuts
    assert set(case.must_cut) <= set(cuts)
    assert any(c + 1 in cuts for c in cuts), cuts          # an adjacent pair: a push of one row
    cov = S.cover(want, b.n)
    assert [c for c in cuts if cov[c] == 0] == []           # no exemptions
    parts = S.parts(case)
    assert sum(p.n for p in parts) == b.n and len(parts) - len(parts) // 2 >= 3      # the decoy hop's rest
    # an engine that drops its state at every cut
    forgetful = S.run_oracle(case.app, parts, fresh_each=True)
    same = len(forgetful) == len(want) and all(
        np.array_equal(getattr(forgetful, f), getattr(want, f)) for f in S.FIELDS)
    assert not same
    print(case.name, "matches", len(want), "forgetful", len(forgetful), "cuts", cuts)


@pytest.mark.parametrize("case", S.CASES, ids=str)
def test_decoy_is_another_stream(case):
    b, d = S.whole(case), S.decoy(case)
    assert d.n == b.n and d.ts.min() >= b.ts.max() + S.DAY
    keys = S.key_count(case, b)
    if keys > 1:
        assert S.key_count(case, d) >= 1.5 * keys, (keys, S.key_count(case, d))
    names = S._names(case.app)
    for name, x in zip(names, d.nulls):
        assert (x is None) == (name == "symbol") and (x is None or x.any()), name
    assert sum(p.n for p in S.decoy_parts(case)) == b.n


def test_stream_properties():
    """what the clock and null cases are about, read off their rows"""
    b = S.whole(S.BY_NAME["machine-c4-late_row"])
    assert 1200 in S.cuts(S.BY_NAME["machine-c4-late_row"]) and b.ts[:1200].max() - b.ts[1200] > S.W
    for name in ("machine-c4-heartbeat", "absent-c4-heartbeat"):
        b = S.whole(S.BY_NAME[name])
        assert b.stream[S.HB_ROW] == -1 and [p.n for p in S.parts(S.BY_NAME[name]) if p.stream[0] == -1] == [1]
        want = S.want(S.BY_NAME[name])
        assert (want.trigger == S.HB_ROW).any()             # the heartbeat fires timers
    b = S.whole(S.BY_NAME["absent-time_back"])
    back = int(np.flatnonzero(np.diff(b.ts) < 0)[0]) + 1
    assert any(back < c <= back + 8 for c in S.cuts(S.BY_NAME["absent-time_back"]))
    for name in ("lanes-count13-time_back", "lanes-c3c-time_back", "lanes-next3-time_back-lateness400"):
        b = S.whole(S.BY_NAME[name])
        assert b.n == 1200 and b.ts[600] == b.ts[599] + 1 - 400
    for name in ("lanes-next3-lateness0", "lanes-next3-time_back-lateness400"):     # the option's promise holds
        case = S.BY_NAME[name]
        b = S.whole(case)
        assert (np.maximum.accumulate(b.ts) - b.ts).max() <= case.engine["max_lateness_ms"]
    for name in ("lanes-next-nulls", "lanes-count13-nulls"):
        flags = [p.nulls[2] is not None for p in S.parts(S.BY_NAME[name])]
        assert not flags[0] and any(flags) and not flags[-1], flags


def test_growth_stream():
    from oracle import OracleEngine
    from parity_util import run_engine
    b = S.growth_stream()
    want = run_engine(OracleEngine, S.GROWTH_Q, [b])
    assert len(want) > 3_000
    cov = S.cover(want, b.n)
    assert cov[S.GROWTH_CUT] > 256 > cov[S.GROWTH_EARLY] > 0     # beyond the first pool of 256 partials, and within it
