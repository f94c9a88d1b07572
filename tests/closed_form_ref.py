"""A row-at-a-time restatement of the two closed-form patterns, for the tests only.

  every e1=A[l] -> e2=B[l' and B.x OP A.x] within T      every_next()    
        e1=A[l] -> e2=B[l' and B.x OP A.x] [within T]    once()          (csrc/once.hip's header,
                                                                          T/query/partition/PatternPartitionTestCase.java)

Plain Python over scalars, None for a null.  It shares no code with lowering.py, the oracle or csrc/: a compare goes
through range_ref._compare, whose domain table is written out per operand type pair, and the boolean forms are walked
here over the compiler's AST by the rules of range_ref.holds (a null result is not TRUE).  `compare` can be replaced,
which test_value_cases.py uses to show that the cases tell a wrong compare from the right one.

Rows are (stream index, timestamp, key, values): values a list over the stream's attributes, None for a null; FLOAT
values are Python floats that hold a binary32 value exactly.  Restated (C/ = modules/siddhi-core/src/main/java/io/
siddhi/core/):

  StreamPreStateProcessor.isExpired        |e1.ts - now| > within drops the partial (C/query/input/stream/state/
                                           StreamPreStateProcessor.java:102-113), before the row is compared
  StreamPreStateProcessor.processAndReturn the pending partials in list order; one that the row completes leaves the
                                           list (:290-331)
  MultiProcessStreamReceiver               for one event the states are visited last state first (C/query/input/
                                           MultiProcessStreamReceiver.java:98-309): B before A, so a row never completes
                                           the partial it starts
  PartitionRuntime.clonePartition          one such runtime per key (C/partition/PartitionRuntime.java:255-308); a row
                                           with a null key reaches none"""
from dataclasses import dataclass, field
from typing import List

import range_ref
from siddhi_amd import compiler as C


@dataclass
class Side:
    """one state of the pattern: its stream (index and definition), the compared attribute's index, and its local
    conditions (A: the filter; B: the conjuncts that read only the arriving row)"""
    stream: int
    defn: C.StreamDefinition
    attr: int
    conds: List[object] = field(default_factory=list)

    @property
    def type(self) -> str:
        return self.defn.attrs[self.attr][1]


def holds(e, d: C.StreamDefinition, values, compare=range_ref._compare) -> bool:
    """range_ref.holds with the compare replaceable"""
    if compare is range_ref._compare:
        return range_ref.holds(e, d, values)
    if isinstance(e, C.And):
        left, right = holds(e.left, d, values, compare), holds(e.right, d, values, compare)
        return left and right
    if isinstance(e, C.Or):
        left, right = holds(e.left, d, values, compare), holds(e.right, d, values, compare)
        return left or right
    if isinstance(e, C.Not):
        return not holds(e.expr, d, values, compare)
    if isinstance(e, C.Compare):
        lt, lv = range_ref._operand(e.left, d, values)
        rt, rv = range_ref._operand(e.right, d, values)
        return compare(e.op, lt, lv, rt, rv)
    return range_ref.holds(e, d, values)


def _passes(side: Side, values, compare) -> bool:
    return all(holds(e, side.defn, values, compare) for e in side.conds)


def every_next(rows, a_filter: Side, b_local: Side, op: str, within: int, partitioned: bool,
               compare=range_ref._compare, expired=lambda dt, within: dt > within):
    """(trigger row, e1 row, e2 row) triples in delivery order.  `expired` is the expiry rule (replaceable like
    `compare`)."""
    a, b = a_filter, b_local
    pending = {}
    out = []
    for j, (s, ts, key, values) in enumerate(rows):
        if partitioned and key is None:
            continue
        lst = pending.setdefault(key if partitioned else 0, [])
        if s == b.stream:
            lst[:] = [i for i in lst if not expired(abs(ts - rows[i][1]), within)]
            if _passes(b, values, compare):
                keep = []
                for i in lst:
                    if compare(op, b.type, values[b.attr], a.type, rows[i][3][a.attr]):
                        out.append((j, i, j))
                    else:
                        keep.append(i)
                lst[:] = keep
        if s == a.stream and _passes(a, values, compare):
            lst.append(j)
    return out


def once(rows, a_filter: Side, b_local: Side, op: str, within, partitioned: bool, compare=range_ref._compare,
         expired=lambda dt, within: dt > within):
    """the form without `every`; within None: no expiry.  Per key: waiting for e1 / e1 bound / done."""
    a, b = a_filter, b_local
    bound, done = {}, set()
    out = []
    for j, (s, ts, key, values) in enumerate(rows):
        if partitioned and key is None:
            continue
        k = key if partitioned else 0
        if k in done:
            continue
        if k in bound:
            if s == b.stream:
                i = bound[k]
                if within is not None and expired(abs(ts - rows[i][1]), within):
                    done.add(k)
                elif _passes(b, values, compare) and compare(op, b.type, values[b.attr], a.type, rows[i][3][a.attr]):
                    out.append((j, i, j))
                    done.add(k)
        elif s == a.stream and _passes(a, values, compare):
            bound[k] = j
    return out
