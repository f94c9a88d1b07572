"""A row-at-a-time restatement of range partition routing, for the tests only.

The host router (runtime._range_mask / _range_route / _broadcast) and the device router (csrc/ranges.hip over the
postfix programs of lowering.lower_ranges) are both vectorised and share lowering._cmp_domain.  This module shares no
code with either: it walks the compiler's AST for one row at a time over Python scalars (None = null), picks the compare
domain from a table written out per operand type pair, and routes the rows one after another with one dictionary of
partition instances.  It restates (C/ = modules/siddhi-core/src/main/java/io/siddhi/core/):

  RangePartitionExecutor.execute           the label if the condition returns TRUE, else null
                                           (C/partition/executor/RangePartitionExecutor.java:38-43)
  PartitionStreamReceiver.receive / send   one executor per range in written order, a send per non-null key, the
                                           instance created on its first send (C/partition/PartitionStreamReceiver.java:
                                           94-100,270-275); no executor: the event goes to every instance that exists
                                           (:83-92,277-281)
  the condition executors                  C/executor/condition/{And,Or,Not,IsNull}ConditionExpressionExecutor.java,
                                           C/executor/condition/compare/**

Rows are (stream index, timestamp, values): values a list over the stream's attributes, None for a null; stream -1 is
a clock row (values None).  FLOAT values are Python floats that hold a binary32 value exactly."""
import struct
from dataclasses import dataclass, field
from typing import List, Optional

from siddhi_amd import compiler as C

# ----------------------------------------------------------------------------------------------- compare domains
# > >= < <= : the executors compare the unboxed operands, `(Float) left > (Long) right`
# (C/executor/condition/compare/greaterthan/GreaterThanCompareConditionExpressionExecutorFloatLong.java:38 and its 63
# siblings in greaterthan/ greaterthanequal/ lessthan/ lessthanequal/), so Java binary numeric promotion picks the type
# (JLS 5.6.2).  One row per <L><R> class name.
RELATIONAL = {
    ("INT", "INT"): "int",          ("INT", "LONG"): "long",        ("INT", "FLOAT"): "float",
    ("INT", "DOUBLE"): "double",    ("LONG", "INT"): "long",        ("LONG", "LONG"): "long",
    ("LONG", "FLOAT"): "float",     ("LONG", "DOUBLE"): "double",   ("FLOAT", "INT"): "float",
    ("FLOAT", "LONG"): "float",     ("FLOAT", "FLOAT"): "float",    ("FLOAT", "DOUBLE"): "double",
    ("DOUBLE", "INT"): "double",    ("DOUBLE", "LONG"): "double",   ("DOUBLE", "FLOAT"): "double",
    ("DOUBLE", "DOUBLE"): "double",
}
# == != : each class converts by hand (C/executor/condition/compare/equal/EqualCompareConditionExpressionExecutor
# <L><R>.java:35-38, notequal/ likewise): IntFloat `.floatValue() == (Float) right`, IntLong `.longValue()`, any with
# Double `.doubleValue()` -- the wider type -- but FloatLong and LongFloat take `.doubleValue()` of both sides
# (EqualCompareConditionExpressionExecutorFloatLong.java:38, ...LongFloat.java:37).
EQUALITY = dict(RELATIONAL)
EQUALITY[("FLOAT", "LONG")] = "double"
EQUALITY[("LONG", "FLOAT")] = "double"

NUMERIC = ("INT", "LONG", "FLOAT", "DOUBLE")


class RefError(Exception):
    pass


def f32(x: float) -> float:
    """the binary32 nearest to the double x, as a Python float"""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def int_to_f32(v: int) -> float:
    """(float) v of a Java int / long: ONE rounding of the exact integer to 24 significant bits, ties to even (JLS
    5.1.2) -- not via a double, which would round 2^60 + 2^36 + 1 to 2^60 + 2^36 first and then, on the tie, to 2^60"""
    a = abs(v)
    nb = a.bit_length()
    if nb > 24:
        sh = nb - 24
        q, rem, half = a >> sh, a & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
        a = q << sh          # <= 24 significant bits (or the next power of two): exact as a double
    return -float(a) if v < 0 else float(a)


def _convert(v, t: str, domain: str):
    if domain in ("int", "long"):
        return v                                   # INT / LONG operands only: exact Python integers
    if t in ("INT", "LONG"):
        return int_to_f32(v) if domain == "float" else float(v)      # int -> float is correctly rounded in Python
    return v                                       # FLOAT widens exactly; DOUBLE only ever meets "double"


# ----------------------------------------------------------------------------------------------- conditions
def _operand(e, d: C.StreamDefinition, values):
    """(type, value or None) of a compare / `is null` operand: an attribute of the row or a constant"""
    if isinstance(e, C.Const):
        if e.type == "FLOAT":
            return "FLOAT", f32(float(e.value))
        if e.type == "DOUBLE":
            return "DOUBLE", float(e.value)
        return e.type, e.value
    if isinstance(e, C.Var):
        ai = d.attr_index(e.attr)
        if ai < 0 or e.stream_ref not in (None, d.id) or e.index is not None:
            raise RefError(f"{e.attr} is not an attribute of {d.id}")
        return d.attrs[ai][1], values[ai]
    raise RefError(f"operand {e!r}")


def _compare(op: str, lt: str, lv, rt: str, rv) -> bool:
    if lt in ("STRING", "BOOL") or rt in ("STRING", "BOOL"):
        # ExpressionParser.parseCompare has only StringString and BoolBool classes, in equal/ and notequal/
        if lt != rt or op not in ("==", "!="):
            raise RefError(f"cannot compare {lt} {op} {rt}")
        domain = None
    else:
        domain = (EQUALITY if op in ("==", "!=") else RELATIONAL)[(lt, rt)]
    if lv is None or rv is None:
        # CompareConditionExpressionExecutor.java:39-43 returns FALSE on a null operand;
        # NotEqualCompareConditionExpressionExecutor.java:37 `left == null || right == null || ...`
        return op == "!="
    if domain is not None:
        lv, rv = _convert(lv, lt, domain), _convert(rv, rt, domain)
    if op == "==":
        return lv == rv
    if op == "!=":
        return lv != rv
    if op == ">":
        return lv > rv
    if op == ">=":
        return lv >= rv
    if op == "<":
        return lv < rv
    if op == "<=":
        return lv <= rv
    raise RefError(f"operator {op}")


def holds(e, d: C.StreamDefinition, values) -> bool:
    """the condition returns Boolean.TRUE on this row (a null result counts as not TRUE everywhere it is read:
    AndConditionExpressionExecutor.java:66-75, Or... likewise, NotConditionExpressionExecutor.java:43-49)"""
    if isinstance(e, C.And):
        left, right = holds(e.left, d, values), holds(e.right, d, values)
        return left and right
    if isinstance(e, C.Or):
        left, right = holds(e.left, d, values), holds(e.right, d, values)
        return left or right
    if isinstance(e, C.Not):
        return not holds(e.expr, d, values)
    if isinstance(e, C.IsNull):          # IsNullConditionExpressionExecutor.java:35-41: any attribute type
        return _operand(e.expr, d, values)[1] is None
    if isinstance(e, C.Var):             # a BOOL attribute is its own condition (VariableExpressionExecutor)
        t, v = _operand(e, d, values)
        if t != "BOOL":
            raise RefError(f"{e.attr} is {t}, not a condition")
        return v is True
    if isinstance(e, C.Compare):
        lt, lv = _operand(e.left, d, values)
        rt, rv = _operand(e.right, d, values)
        return _compare(e.op, lt, lv, rt, rv)
    raise RefError(f"condition {e!r}")


# ----------------------------------------------------------------------------------------------- routing
def _java_string(v, t: str) -> Optional[str]:
    """String.valueOf of a value partition key (C/partition/executor/ValuePartitionExecutor.java:34-39); INT, LONG,
    STRING and BOOL keys only"""
    if v is None:
        return None
    if t == "BOOL":
        return "true" if v else "false"
    if t in ("INT", "LONG", "STRING"):
        return str(v)
    raise RefError(f"value keys of type {t} are outside this restatement")


def _streams_read(node, out: set):
    """ids of the streams the query's pattern reads: every state element with a stream id, however nested"""
    if isinstance(node, (list, tuple)):
        for x in node:
            _streams_read(x, out)
    elif hasattr(node, "__dataclass_fields__"):
        sid = getattr(node, "stream_id", None)
        if sid is not None:
            out.add(sid)
            return
        for name in node.__dataclass_fields__:
            _streams_read(getattr(node, name), out)


@dataclass
class Routed:
    rows: List[tuple] = field(default_factory=list)   # (event index, stream, key, ts, values tuple or None)
    src: List[int] = field(default_factory=list)      # per routed row: the input row it is a copy of
    keys: List[str] = field(default_factory=list)     # the dictionary in creation order (id = position)


def route(app: C.SiddhiApp, rows, keys=(), base_index: int = 0, indices=None, broadcast: bool = True) -> Routed:
    """Route rows through the app's first partition, one row after another.  keys: the instances that exist already,
    in creation order.  indices: the event index per row (default base_index + position).  broadcast=False leaves the
    rows of unpartitioned streams as they are (what a router below the broadcast step sees)."""
    part = app.partitions[0]
    sids = list(app.streams.keys())
    value_attr = {sids.index(sid): app.streams[sid].attr_index(attr) for sid, attr in part.keys}
    ranges = {sids.index(sid): rl for sid, rl in part.ranges.items()}
    read = set()
    for q in part.queries:
        _streams_read(q.input.element, read)
    everyone = {sids.index(sid) for sid in read} - set(value_attr) - set(ranges) if broadcast else set()
    ids = {k: i for i, k in enumerate(keys)}
    out = Routed()

    def instance(key: str) -> int:        # PartitionRuntime.cloneIfNotExist: created the moment a row needs it
        if key not in ids:
            ids[key] = len(ids)
        return ids[key]

    for pos, (s, ts, values) in enumerate(rows):
        index = base_index + pos if indices is None else int(indices[pos])
        vt = None if values is None else tuple(values)

        def emit(stream, key):
            out.rows.append((index, stream, key, ts, vt))
            out.src.append(pos)
        if s in ranges:
            d = app.streams[sids[s]]
            held = [label for cond, label in ranges[s] if holds(cond, d, values)]
            for label in held:            # one send per holding range, written order
                emit(s, instance(label))
            if not held and app.playback:
                emit(-1, -1)              # InputHandler.send moved the clock before the receiver dropped the row
        elif s in value_attr:
            d = app.streams[sids[s]]
            ks = _java_string(values[value_attr[s]], d.attrs[value_attr[s]][1])
            emit(s, -1 if ks is None else instance(ks))
        elif s in everyone:
            for k in range(len(ids)):     # the instances earlier rows created, in creation order
                emit(s, k)
        else:
            emit(s, -1)
    out.keys = list(ids)
    return out
