"""Which route of the general family ran (siddhi_amd/csrc/partial.hip: sg_partial_push for partial lanes, and the
sequence lanes behind it; interp.hip run_machine for the per-key machine), push by push, on small streams against the
oracle.

sg_partial_push returns 0 to decline a stream and the per-key machine then takes it, exactly: every parity test passes
whichever route ran.  So every case here also asserts, per push, the names of the kernels the handle timed
(timing().kernels(): the driver's kbeg(...) marks, in launch order):

  partial lanes   [pred] route key_sort pack start_rows [wait_sum] partial_lanes [match_order] carry
                  pred: the query has an event-local filter; wait_sum: the rule has wait slots (chain.h pp_wait_rule)
                  and the push holds no null flags; match_order: the push delivers a match
  sequence lanes  [pred] route key_sort pack sequence_units (sequence_lanes sequence_fix)+ [match_order] carry
                  the pair repeats when the push outgrew its match space and was rerun
  the machine     route key_sort [pred] nfa_keys | nfa_units [match_order]
  record sort     "route key_sort" carry the rows' hot fields through the key sort as one 16-byte record; a push with a
  backs out       timestamp more than 2^31 ms from its first row runs them again on the gather path: both twice, pack once

Streams are about 2,000 rows over 7 keys in three pushes cut at uneven places (the handle keeps at most 24 marks per
push)."""
import numpy as np
import pytest

from oracle import OracleEngine
from parity_util import assert_same, run_engine
from test_partial_lanes import HEAD, SEQ_SHAPES, SHAPES, small_batch, split

pytestmark = pytest.mark.gpu

LANES = ("route", "key_sort", "pack", "start_rows", "partial_lanes", "carry")
SEQ = ("route", "key_sort", "pack", "sequence_units", "sequence_lanes", "sequence_fix", "carry")
OTHER_ROUTES = ("nfa_keys", "nfa_units", "sequence_units", "sequence_lanes", "sequence_fix")
# shapes whose rule has wait slots: some state's filter is one fast compare of the arriving row's 4-byte attribute with
# an operand fixed while the partial waits there (filter_cross: two terms at e2, arithmetic at e3)
WAIT_SUM = {name: name != "filter_cross" for name in SHAPES}
# every shape's start state has an event-local filter (`e1=S[v>50]`)
PRED = {name: True for name in list(SHAPES) + list(SEQ_SHAPES)}
DAY = 86_400_000


class _Witness:
    """GpuEngine wrapper recording, per push, the names of the kernels the handle timed."""
    kw = {}
    log = []

    def __init__(self, ctx):
        from siddhi_amd._native import GpuEngine
        self.e = GpuEngine(ctx, **_Witness.kw)

    def push(self, b):
        self.e.push(b)
        _Witness.log.append([name for name, _ in self.e.handle.timing().kernels()])

    def fetch(self):
        return self.e.fetch()

    def close(self):
        self.e.close()


class _Oracle:
    """OracleEngine wrapper keeping every fetch apart (matches per push)."""
    outs = []

    def __init__(self, ctx):
        self.e = OracleEngine(ctx)

    def push(self, b):
        self.e.push(b)

    def fetch(self):
        o = self.e.fetch()
        _Oracle.outs.append(o)
        return o

    def close(self):
        self.e.close()


def drive(q, batches, check, **kw):
    """GpuEngine against the oracle over `batches`, bit for bit, then check(i, names, matches the oracle delivered for
    push i) for every push.  Returns the kernel names per push."""
    _Oracle.outs = []
    want = run_engine(_Oracle, q, batches)
    per = [len(o) for o in _Oracle.outs]
    _Oracle.outs = []
    _Witness.kw, _Witness.log = kw, []
    got = run_engine(_Witness, q, batches)
    log, _Witness.log = _Witness.log, []
    assert len(want) > 0
    assert_same(got, want)
    assert len(log) == len(batches) == len(per)
    for i, names in enumerate(log):
        assert len(names) < 24, names   # (the handle's mark limit: a longer push would be cut short)
        check(i, names, per[i])
    return log


def once_each(names, which, where):
    for k in which:
        assert names.count(k) == 1, f"{where}: '{k}' {names.count(k)} times in {names}"


def none_of(names, which, where):
    for k in which:
        assert k not in names, f"{where}: '{k}' in {names}"


def check_lanes(name, wait_sum=None):
    """one partial-lane push; wait_sum: per push (default: the shape's, every push)"""
    def check(i, names, emitted):
        where = f"{name} push {i + 1}"
        once_each(names, LANES, where)
        none_of(names, OTHER_ROUTES, where)
        assert names.count("match_order") == (1 if emitted else 0), f"{where}: {emitted} matches, {names}"
        assert names.count("pred") == (1 if PRED[name] else 0), f"{where}: {names}"
        ws = WAIT_SUM[name] if wait_sum is None else wait_sum[i]
        assert names.count("wait_sum") == (1 if ws else 0), f"{where}: {names}"
    return check


def stream(name, n=2000, vmax=100, rate=4):
    return small_batch(n, 7, vmax, rate, seed=sum(name.encode()) + 1)


# ---- 1. partial lanes

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_partial_lanes_route(name):
    """sg_partial_push, mode 1, every shape of the family; for `next` the second push is a single row"""
    cuts = [700, 701] if name == "next" else [613, 1307]
    drive(HEAD + SHAPES[name], split(stream(name), cuts), check_lanes(name), force_general=True)


# ---- 2. sequence lanes

@pytest.mark.parametrize("name", sorted(SEQ_SHAPES))
def test_sequence_lanes_route(name):
    """sg_partial_push, mode 2 (seq_lanes_push), every shape of the family"""
    def check(i, names, emitted):
        where = f"{name} push {i + 1}"
        once_each(names, SEQ, where)
        none_of(names, ("start_rows", "partial_lanes", "wait_sum", "nfa_keys", "nfa_units"), where)
        assert names.count("match_order") == (1 if emitted else 0), f"{where}: {emitted} matches, {names}"
        assert names.count("pred") == (1 if PRED[name] else 0), f"{where}: {names}"
    drive(HEAD + SEQ_SHAPES[name], split(stream(name), [613, 1307]), check)


# ---- 3. the machine

@pytest.mark.parametrize("family,name", [("pattern", "c3c"), ("sequence", "seq_c3b")])
def test_machine_route(family, name):
    """partial_lanes=-1 keeps the stream off both lane routes: run_machine"""
    def check(i, names, emitted):
        where = f"{name} push {i + 1}"
        assert "nfa_keys" in names or "nfa_units" in names, f"{where}: {names}"
        none_of(names, ("partial_lanes", "sequence_lanes", "pack"), where)
    q = HEAD + (SHAPES if family == "pattern" else SEQ_SHAPES)[name]
    drive(q, split(stream(name), [613, 1307]), check, force_general=True, partial_lanes=-1)


# ---- 4. the record sort backs out

def test_record_sort_falls_back_to_gather():
    """`next` takes the record sort (its one non-local filter reads one 4-byte slot; only the start state is local).
    The last row of push 2 lies 30 days after the push's first row: its offset does not fit the record's 32 bits,
    k_pp_rec raises the flag and the push runs route and key_sort again on the gather path.  The row fails the start
    filter and expires its key's partials, so it is not carried: pushes 1 and 3 keep the record sort."""
    b = stream("next")
    b.ts[1306] += 30 * DAY
    b.cols[2][1306] = 0

    def check(i, names, emitted):
        where = f"push {i + 1}"
        k = 2 if i == 1 else 1
        assert names.count("route") == k and names.count("key_sort") == k, f"{where}: {names}"
        once_each(names, ("pred", "pack", "start_rows", "wait_sum", "partial_lanes", "carry"), where)
        none_of(names, OTHER_ROUTES, where)
        assert names.count("match_order") == (1 if emitted else 0), f"{where}: {emitted} matches, {names}"
    drive(HEAD + SHAPES["next"], split(b, [613, 1307]), check, force_general=True)


# ---- 5. nulls

def test_nulls_stay_on_partial_lanes():
    """null flags on the compared column in push 2 only: that push and, through the carried rows, the third pack a null
    mask (gather path) and run without wait summaries (a null row passes `!=`); all three stay on partial lanes"""
    parts = split(stream("next"), [613, 1307])
    rng = np.random.default_rng(3)
    parts[1].nulls[2] = (rng.random(parts[1].n) < 0.05).astype(np.uint8)
    assert WAIT_SUM["next"]
    drive(HEAD + SHAPES["next"], parts, check_lanes("next", wait_sum=[True, False, False]), force_general=True)


# ---- 6. a sequence push that outgrows its match space

def test_sequence_match_space_rerun(monkeypatch):
    """SG_DEBUG_SQ_MATCH_CAP=16: the first attempt of every push has 16 match slots, one lane's chunk, so the push is
    rerun from the unchanged start states with more space"""
    monkeypatch.setenv("SG_DEBUG_SQ_MATCH_CAP", "16")

    def check(i, names, emitted):
        where = f"push {i + 1}"
        once_each(names, ("route", "key_sort", "pack", "sequence_units", "carry"), where)
        assert names.count("sequence_lanes") == names.count("sequence_fix") >= 1, f"{where}: {names}"
        if i == 0:
            assert emitted > 16 and names.count("sequence_lanes") >= 2, f"{where}: {emitted} matches, {names}"
        none_of(names, ("partial_lanes", "nfa_keys", "nfa_units"), where)
    drive(HEAD + SEQ_SHAPES["seq_next"], split(stream("seq_next"), [613, 1307]), check)


# ---- 7. sub-pushes

def test_push_past_the_row_budget_runs_as_two_sub_pushes(monkeypatch):
    """SG_DEBUG_PP_ROW_BUDGET=1000, pushes of 500, 1,200 and 300 rows: the second has more rows than the budget leaves
    beside the carried ones (`next`, within 40 ms at 4 rows per ms: at most a few hundred) and runs as two sub-pushes,
    every stage twice; the others fit"""
    monkeypatch.setenv("SG_DEBUG_PP_ROW_BUDGET", "1000")

    def check(i, names, emitted):
        where = f"push {i + 1}"
        k = 2 if i == 1 else 1
        for x in LANES + ("pred", "wait_sum"):
            assert names.count(x) == k, f"{where}: '{x}' {names.count(x)} times in {names}"
        none_of(names, OTHER_ROUTES, where)
    drive(HEAD + SHAPES["next"], split(stream("next"), [500, 1700]), check, force_general=True)
