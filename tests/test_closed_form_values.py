"""Compared values from the edge pools of value_cases.py on every route of the every-next closed form and on the once
route, on the GPU: all four value types (the 8-byte instantiations engine_i64 / engine_f64 included), all four
operators, stack and list mode, on the tiled walker with and without a stream column, the sort partition, the
unpartitioned search and walker, the HBM-list redo, wide records (24 bytes for LONG and DOUBLE), the exact walker after
a key's time went back, the value carry between pushes, and two streams.

Every case is compared with the oracle field for field and bit for bit (-0.0 and NaN payloads count), its
(trigger, e1.id, e2.id) with the row-at-a-time reference (closed_form_ref.py), and the route is read off the kernels
the handle timed.  test_value_cases.py guards the cases themselves on the CPU."""
import pytest

import value_cases as V
from oracle import OracleEngine
from parity_util import assert_same, run_engine

pytestmark = pytest.mark.gpu


def check_route(case, log):
    names = [n for push, _ in log for n in push]
    spilled = sum(s for _, s in log)
    msg = f"{case.name}: {log}"
    assert "group_walk" not in names, msg
    if case.route == "once":
        assert all("once_match" in push for push, _ in log), msg
        return
    if case.route == "search":
        assert "nge_search" in names and "walk_count" not in names, msg
        return
    assert all("walk_count" in push for push, _ in log), msg         # the tiled walker ran in every push
    assert "nge_search" not in names, msg
    assert ("key_sort" in names) == (case.route == "sorted"), msg
    if case.route == "redo":
        assert spilled > 0, msg
    elif case.route == "wide":
        # the narrow attempt of the push that holds the gap returns false after its predicate pass; the wide one starts over
        assert any(push.count("pred") == 2 for push, _ in log), msg
    elif case.route == "time_back":
        # the count pass reports the order error and runs again with those keys on the exact walker
        assert any(push.count("walk_count") == 2 for push, _ in log), msg
    elif case.route == "carry":
        assert len(log) == 4 and all("carry" in push for push, _ in log[:-1]), msg


@pytest.mark.parametrize("case", V.CLOSED, ids=str)
def test_closed_form_values(case):
    want = run_engine(OracleEngine, case.app, V.pushes(case))
    ref = V.reference(case)
    assert len(want) >= case.floor and V.triples(want) == ref
    for stream_column in (True, False) if case.no_stream_column else (True,):
        got, log = V.run_gpu(case, stream_column)
        print(case.name, "stream column" if stream_column else "no stream column", log)
        assert_same(got, want)
        assert V.triples(got) == ref
        check_route(case, log)
