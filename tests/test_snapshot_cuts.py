"""sg_snapshot / sg_restore at every cut, on every route and handle state (include/siddhi_gpu.h): a restored
handle continues as if the stream had never stopped.

The cases of snapshot_cases.py (test_snapshot_cases.py guards them on the CPU: every cut is one that state has to cross)
run in four hop modes -- a fresh handle per cut, two handles playing ping-pong, a handle that has run another stream
before, and a blob that went through one more handle with nothing pushed -- and the concatenated output must be the
oracle's over the uninterrupted stream, bit for bit.  Every push is also asserted to have run on the case's route, by
the kernel names the handle timed: a restore must not bounce a stream to the per-key machine unnoticed.

Then, for one case per state kind and lane mode: blobs are deterministic, the two-call protocol gives the bytes of one
call, and a blob that fails to restore leaves a handle that sg_reset makes good again (the header's contract).  Blob
bytes are never altered: carried key ids, list indices and state positions are trusted device data."""
import ctypes as ct
import dataclasses

import numpy as np
import pytest

import snapshot_cases as S
from parity_util import assert_same, context
from test_closed_form_values import check_route
from test_lane_routes import LANES, OTHER_ROUTES, SEQ, WAIT_SUM, check_lanes, none_of, once_each

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- which route ran
def emitted_per_push(case):
    """matches the oracle delivers at the rows of each push"""
    t = S.want(case).trigger.astype(np.int64)
    edges = [0] + S.cuts(case) + [S.whole(case).n]
    return [int(((t >= lo) & (t < hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]


def check_routes(case, tr, first=0):
    """every push of the trace (the pushes of the case from number `first` on) ran on the case's route"""
    emitted = emitted_per_push(case)[first:]
    assert len(tr.log) == len(emitted) == len(tr.restored)
    msg = f"{case.name}: {tr.log}"
    if case.family in ("every", "once"):
        src = case.source
        # (the carry case's own check counts its four pushes: here every push but the last carries)
        check_route(dataclasses.replace(src, route="tiled" if src.route == "carry" else src.route), tr.log)
        if src.route != "search" and case.family == "every":
            assert all("carry" in names for names, _ in tr.log[:-1]), msg
        return
    for i, (names, _) in enumerate(tr.log):
        where = f"{case.name} push {first + i + 1}"
        assert len(names) < 24, names
        if case.family == "absent":
            assert "abs_roles" in names or "abs_sequential" in names, f"{where}: {names}"
            none_of(names, ("nfa_keys", "nfa_units"), where)
        elif case.family == "machine":
            assert "nfa_keys" in names or "nfa_units" in names, f"{where}: {names}"
            none_of(names, ("partial_lanes", "sequence_lanes", "pack", "abs_roles", "abs_sequential"), where)
        elif case.family == "lanes":
            # wait summaries run only while neither the push nor the carried rows may hold a null: a restored handle
            # takes its carried rows as possibly null (sg_partial_restore), and every cut here carries rows
            fresh = not tr.restored[i] and all(x is None for p in S.parts(case)[:first + i + 1] for x in p.nulls)
            if case.shape in S.SHAPES:
                ws = WAIT_SUM[case.shape] and fresh
                check_lanes(case.shape, wait_sum=[ws] * (i + 1))(i, names, emitted[i])
            else:
                once_each(names, LANES, where)
                none_of(names, OTHER_ROUTES, where)
                assert names.count("match_order") == (1 if emitted[i] else 0), f"{where}: {emitted[i]} matches, {names}"
        else:
            once_each(names, SEQ, where)
            none_of(names, ("start_rows", "partial_lanes", "wait_sum", "nfa_keys", "nfa_units"), where)
            assert names.count("match_order") == (1 if emitted[i] else 0), f"{where}: {emitted[i]} matches, {names}"
            assert names.count("pred") == 1, f"{where}: {names}"
    if case.sequential:
        assert any("abs_sequential" in names for names, _ in tr.log), msg


# ---------------------------------------------------------------------------------------------- the four hop modes
@pytest.mark.parametrize("mode", list(S.HOPS))
@pytest.mark.parametrize("case", S.CASES, ids=str)
def test_restored_handle_continues(case, mode):
    want = S.want(case)
    assert len(want) >= case.floor > 0
    tr = S.HOPS[mode](case)
    first = len(S.parts(case)) - len(tr.log)
    print(case.name, mode, len(tr.log), "pushes", len(want), "matches")
    assert first == 0
    assert_same(tr.output(), want)
    check_routes(case, tr)


# ---------------------------------------------------------------------------------------------- growth
def _growth_parts(cuts):
    return S.V.pieces(S.growth_stream(), cuts)


def _growth_engine():
    from siddhi_amd._native import GpuEngine
    return GpuEngine(context(S.GROWTH_Q), **S.GROWTH_ENGINE)


def _growth_want():
    return S.run_oracle(S.GROWTH_Q, [S.growth_stream()])


def _after(out, row):
    keep = out.trigger.astype(np.int64) >= row
    return S.Outputs(*[getattr(out, f)[keep] for f in S.FIELDS])


def test_grown_geometry_restores_into_a_fresh_handle():
    """test_capacity.py's skewed key: by row 1,700 the machine's pools have grown past the 256 partials a handle opens
    with; the blob brings its geometry along and a handle of the default geometry adopts it (sg_general_restore)"""
    head, tail = _growth_parts([S.GROWTH_CUT])
    a = _growth_engine()
    outs = [S.push(a, head)]
    blob = a.snapshot()
    a.close()
    b = _growth_engine()
    b.restore(blob)
    outs.append(S.push(b, tail))
    b.close()
    assert_same(S.cat(outs), _growth_want())


def test_ungrown_blob_restores_into_a_grown_handle():
    """the reverse: the blob of row 200 (first geometry) into the handle that has grown since; it shrinks back, runs the
    rest of the stream from row 200, and grows again on the way"""
    early, mid, tail = _growth_parts([S.GROWTH_EARLY, S.GROWTH_CUT])
    a = _growth_engine()
    S.push(a, early)
    small = a.snapshot()
    S.push(a, mid)
    grown = a.snapshot()
    assert len(grown) > 4 * len(small)          # (the pools grow fourfold at a time)
    a.restore(small)
    outs = [S.push(a, mid), S.push(a, tail)]
    a.close()
    assert_same(S.cat(outs), _after(_growth_want(), S.GROWTH_EARLY))


# ---------------------------------------------------------------------------------------------- blob properties
BLOBS = [S.BY_NAME[n] for n in S.BLOB_CASES]


def _blobs(case):
    """the blob after every push but the last of one handle over the case's pushes"""
    eng, out = S.open_engine(case), []
    for p in S.parts(case)[:-1]:
        S.push(eng, p)
        out.append(eng.snapshot())
    eng.close()
    return out


@pytest.mark.parametrize("case", BLOBS, ids=str)
def test_blobs_are_deterministic(case):
    """two handles fed the same pushes give the same bytes at every cut: no uninitialised device memory, struct padding
    or capacity tail reaches a blob, on any route"""
    a, b = _blobs(case), _blobs(case)
    assert len(a) == len(S.cuts(case)) and min(len(x) for x in a) > 64
    for k, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), (case.name, k, len(x), len(y))
        if x != y:
            at = int(np.flatnonzero(np.frombuffer(x, np.uint8) != np.frombuffer(y, np.uint8))[0])
            raise AssertionError(f"{case.name}: blobs after push {k + 1} differ first at byte {at} of {len(x)}")


@pytest.mark.parametrize("case", BLOBS, ids=str)
def test_snapshot_call_protocol(case):
    """a size query followed by a copy gives the bytes of one call with a large buffer; a buffer one byte too small
    reports the size and is left untouched, and the full call after it still gives the same bytes"""
    eng = S.open_engine(case)
    mid = len(S.parts(case)) // 2
    for p in S.parts(case)[:mid]:
        S.push(eng, p)
    h = eng.handle
    two_calls = h.snapshot()
    n = len(two_calls)
    size = ct.c_size_t()
    big = ct.create_string_buffer(b"\xa5" * (n + 4096), n + 4096)
    h.check(h.lib.sg_snapshot(h.h, big, n + 4096, ct.byref(size)))
    assert size.value == n and big.raw[:n] == two_calls and big.raw[n:] == b"\xa5" * 4096
    short = ct.create_string_buffer(b"\xa5" * n, n)
    size = ct.c_size_t()
    h.check(h.lib.sg_snapshot(h.h, short, n - 1, ct.byref(size)))
    assert size.value == n and short.raw == b"\xa5" * n
    full = ct.create_string_buffer(n)
    h.check(h.lib.sg_snapshot(h.h, full, n, ct.byref(size)))
    assert size.value == n and full.raw == two_calls
    assert h.snapshot() == two_calls
    eng.close()


@pytest.mark.parametrize("case", BLOBS, ids=str)
def test_failed_restore_then_reset(case):
    """'On error call sg_reset before reuse': every truncated blob and one with a byte too many is refused; after a
    reset the handle runs the whole stream from row 0 like a new one, then takes the intact blob and continues"""
    from siddhi_amd._native import SgError
    want, ps = S.want(case), S.parts(case)
    mid = len(ps) // 2
    src = S.open_engine(case)
    head = [S.push(src, p) for p in ps[:mid]]
    blob = src.snapshot()
    src.close()
    n = len(blob)
    assert n > 64
    bad = [blob[:k] for k in (0, 7, 8, 12, 31, n // 4, n // 2, n - 1)] + [blob + b"\0"]
    eng = S.open_engine(case)
    for k, x in enumerate(bad):
        if k % 3 == 1:       # (some of the refused blobs meet a handle that holds state)
            for p in ps[:2]:
                S.push(eng, p)
        with pytest.raises(SgError):
            eng.restore(x)
        eng.handle.reset()
    with pytest.raises(SgError):
        eng.restore(bad[5])
    eng.handle.reset()
    tr = S.Trace()
    for p in ps:
        S.push(eng, p, tr)
    assert_same(tr.output(), want)
    eng.restore(blob)
    tr2 = S.Trace()
    for p in ps[mid:]:
        S.push(eng, p, tr2, True)
    eng.close()
    assert_same(S.cat(head + tr2.outs), want)
    check_routes(case, tr2, first=mid)
