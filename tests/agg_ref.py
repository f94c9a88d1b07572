"""Row-at-a-time restatement of the selector's attribute aggregators and group by, over Python scalars: the expected
values of the aggregate tests.  Shares no code with the lowering or the kernels.

What is restated (C/ = modules/siddhi-core/src/main/java/io/siddhi/core/):
  QuerySelector.processGroupBy / processNoGroupBy (C/query/selector/QuerySelector.java:125-216): per match in delivery
      order, the group's aggregators take the match's argument and return their running value; `having` runs after
      that over the output row, so a dropped match has still updated its aggregators.
  GroupByKeyGenerator.constructEventKey (C/query/selector/GroupByKeyGenerator.java:63-73): the group is the
      concatenated toString of the group-by values; state is per partition instance first.
  Count / Sum / Avg / Min / Max AttributeAggregator.processAdd (C/query/selector/attribute/aggregator/*.java).

A record is (partition key, [group values], [argument per aggregate]) with None for null, int for INT / LONG / STRING
ids, float for DOUBLE and a float already rounded to binary32 for FLOAT.  `wrong` names one deliberately wrong rule
(the guard in test_agg_cases.py checks that each changes some case)."""
import math
import struct

WRONG_RULES = ("fp_sum_f32", "reversed_sum", "avg_counts_null", "count_skips_null", "ieee_fmax", "nan_replaces",
               "later_zero_replaces", "reset_per_push", "having_first", "numeric_groups", "shared_keys")

_M64 = (1 << 64) - 1


def f32(x: float) -> float:
    """x rounded to binary32 (overflow to an infinity, as a narrowing cast)"""
    if math.isnan(x) or math.isinf(x):
        return x
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def wrap64(x: int) -> int:
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def java_string(v, t, numeric=False):
    """String.valueOf identity of one group-by value: equal strings <=> equal results here."""
    if v is None:
        return ("null",)
    if t in ("FLOAT", "DOUBLE"):
        if math.isnan(v):
            return ("NaN",)
        if numeric:                       # (wrong rule: -0.0 == 0.0)
            return ("f", v + 0.0 if v != 0 else 0.0)
        return ("f", struct.pack("<d", v))   # bits keep -0.0 and 0.0 apart; every other value has its own string
    return ("i", int(v))


class _Agg:
    def __init__(self, name, atype, wrong):
        self.name, self.atype, self.wrong = name, atype, wrong
        self.count = 0          # count: matches; sum / avg: added values
        self.isum = 0
        self.fsum = 0.0
        self.ext = None
        self.added = []         # (wrong rule reversed_sum)

    def add(self, v):
        n, w = self.name, self.wrong
        fp = self.atype in ("FLOAT", "DOUBLE")
        if n == "count":
            if v is None and w == "count_skips_null":
                return self.count
            self.count += 1
            return self.count
        if v is None:
            if n == "avg" and w == "avg_counts_null":
                self.count += 1
            if n in ("min", "max"):
                return self.ext
            if self.count == 0:
                return None
            if n == "sum":
                return self.fsum if fp else self.isum
            return self.fsum / self.count
        if n in ("sum", "avg"):
            self.count += 1
            if fp or n == "avg":
                x = float(v)              # (Float).doubleValue() / (double) of an int or long
                if w == "fp_sum_f32" and fp:
                    self.fsum = f32(f32(self.fsum) + f32(x))
                elif w == "reversed_sum" and fp:
                    self.added.append(x)
                    s = 0.0
                    for y in reversed(self.added):
                        s += y
                    self.fsum = s
                else:
                    self.fsum += x
            else:
                self.isum = wrap64(self.isum + int(v))
            if n == "sum":
                return self.fsum if fp else self.isum
            return self.fsum / self.count
        # min / max: `maxValue == null || maxValue < value` (MaxAttributeAggregator.java:191); min with >
        if self.ext is None:
            self.ext = v
            return self.ext
        if w == "ieee_fmax" and fp:
            if math.isnan(self.ext):
                self.ext = v
            elif not math.isnan(v):
                self.ext = max(self.ext, v) if n == "max" else min(self.ext, v)
            return self.ext
        if w == "nan_replaces" and fp and math.isnan(v):
            self.ext = v
            return self.ext
        if w == "later_zero_replaces" and fp and v == 0 and self.ext == 0:
            self.ext = v
            return self.ext
        if (self.ext < v) if n == "max" else (self.ext > v):
            self.ext = v
        return self.ext


def fold(pushes, aggs, group_types, partitioned, having=None, wrong=None):
    """pushes: list of lists of records; aggs: [(name, argument TYPE)].  Returns per push the list of
    (record index within the push, [aggregate values]) of the matches `having` keeps."""
    state = {}
    out = []
    for recs in pushes:
        if wrong == "reset_per_push":
            state = {}
        rows = []
        for i, (pkey, gvals, args) in enumerate(recs):
            gk = tuple(java_string(v, t, wrong == "numeric_groups") for v, t in zip(gvals, group_types))
            key = (pkey if partitioned and wrong != "shared_keys" else 0, gk)
            if key not in state:
                state[key] = [_Agg(n, t, wrong) for n, t in aggs]
            if wrong == "having_first" and having is not None:
                # (wrong rule: the filter decides on the values before this match, and a dropped match adds nothing)
                import copy
                trial = [copy.deepcopy(a).add(v) for a, v in zip(state[key], args)]
                if not having(trial):
                    continue
            vals = [a.add(v) for a, v in zip(state[key], args)]
            if having is None or having(vals):
                rows.append((i, vals))
        out.append(rows)
    return out


def result_type(name, atype):
    if name == "count":
        return "LONG"
    if name == "sum":
        return "LONG" if atype in ("INT", "LONG") else "DOUBLE"
    if name == "avg":
        return "DOUBLE"
    return atype


def bits(v, t):
    """a value as the 64-bit word the engines deliver (sg_matches.vals)"""
    if t == "FLOAT":
        return struct.unpack("<I", struct.pack("<f", v))[0]
    if t == "DOUBLE":
        return struct.unpack("<q", struct.pack("<d", v))[0]
    return int(v)


def from_bits(b, t):
    b = int(b)
    if t == "FLOAT":
        return struct.unpack("<f", struct.pack("<I", b & 0xFFFFFFFF))[0]
    if t == "DOUBLE":
        return struct.unpack("<d", struct.pack("<q", b))[0]
    return b


def same_value(got_bits, want, t):
    """bit for bit, any NaN equal to any NaN of the same width"""
    if t in ("FLOAT", "DOUBLE") and math.isnan(want):
        return math.isnan(from_bits(got_bits, t))
    return int(got_bits) == bits(want, t)
