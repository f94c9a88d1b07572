"""Reference and case tables of test_select_cases.py (CPU guard) and test_select_values.py (GPU): the `select` / `having`
pass behind every route, at edge values.

The reference is a plain restatement of the reference's executors as Python scalars: the math executors
(C/executor/math/**: operands converted to the result type as Number.xxxValue() does, int / long wrap, truncating
division, dividend-signed remainder, null on a null operand or a zero divisor, FLOAT arithmetic in binary32), the result
type of ExpressionParser.parseArithmeticOperationResultType, the compare executors (C/executor/condition/compare/**: a
null operand is false except under `!=`; `> >= < <=` by Java binary promotion, so long vs float compares in float; `==` /
`!=` of a FLOAT-LONG pair in double) and And / Or / Not / IsNull (a null or false operand of `not` gives true).  It shares
no code with the lowering, the oracle or the kernels.

A case never restates a pattern rule.  Its pattern text is used twice: the *plain twin* selects the matched attributes
themselves, the *expression twin* selects expressions over them (and may carry a `having`).  The oracle on the plain twin
gives the matched base values per record; the reference evaluates the expressions on those; an engine's output on the
expression twin must equal that (nulls agree, a NaN equals any NaN of its width, everything else bit for bit)."""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List, Optional

import numpy as np

from siddhi_amd import synth
from siddhi_amd.runtime import Batch, Outputs

T0 = 1_700_000_000_000
TYPES = ("INT", "LONG", "FLOAT", "DOUBLE")
MATH_OPS = ("+", "-", "*", "/", "%")
CMP_OPS = ("==", "!=", ">", ">=", "<", "<=")
RANK = {"INT": 0, "LONG": 1, "FLOAT": 2, "DOUBLE": 3}
COLTYPE = {"id": "LONG", "seq": "LONG", "symbol": "STRING", "a": "INT", "b": "LONG", "f": "FLOAT", "d": "DOUBLE",
           "v": "INT", "w": "INT", "flag": "INT", "x": "INT", **{f"c{k}": "INT" for k in range(16)}}
NP = {"INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64, "STRING": np.int32}

# the rules a wrong implementation could follow instead (test_select_cases.py: each changes some case's answer)
WRONG_RULES = ("long_to_float_through_double", "floor_division", "remainder_signed_by_divisor",
               "min_by_minus_one_saturates", "float_arithmetic_in_double", "zero_divisor_divides",
               "nan_divisor_is_null", "float_long_equal_in_float", "long_float_order_in_double", "null_not_equal_is_false")
JAVA = frozenset()


# ---------------------------------------------------------------------------------------------- arithmetic
def _wrap(x, bits):
    m = 1 << bits
    x %= m
    return x - m if x >= m >> 1 else x


def _jdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _f32(x, rules=JAVA):
    """Number.floatValue(): an int / long rounds once (numpy's int64 -> float32 cast; through a double it rounds twice)"""
    if _is_int(x):
        return np.float32(float(int(x))) if "long_to_float_through_double" in rules else np.float32(np.int64(x))
    return np.float32(x)


def _jmath(op, a, b, t, rules=JAVA):
    """`a op b` of the math executor of result type t; a / b Python ints or floats (a FLOAT is a float holding a binary32
    value), None = null"""
    if a is None or b is None:
        return None
    if t in ("INT", "LONG"):
        bits = 32 if t == "INT" else 64
        a, b = int(a), int(b)
        if op in "/%" and b == 0:
            return None
        r = {"+": a + b, "-": a - b, "*": a * b}.get(op)
        if op == "/":
            r = a // b if "floor_division" in rules else _jdiv(a, b)
            if "min_by_minus_one_saturates" in rules and r == 1 << (bits - 1):
                r -= 1
        elif op == "%":
            r = a % b if "remainder_signed_by_divisor" in rules else a - b * _jdiv(a, b)
        return _wrap(r, bits)
    with np.errstate(all="ignore"):
        if t == "FLOAT" and "float_arithmetic_in_double" not in rules:
            x, y = _f32(a, rules), _f32(b, rules)
        else:
            x, y = np.float64(a), np.float64(b)
        if op in "/%":
            if y == 0 and "zero_divisor_divides" not in rules:
                return None
            if y != y and "nan_divisor_is_null" in rules:
                return None
        r = {"+": x + y, "-": x - y, "*": x * y, "/": x / y}.get(op) if op != "%" else np.fmod(x, y)
        return float(np.float32(r)) if t == "FLOAT" else float(r)


def _jcmp(op, a, ta, b, tb, rules=JAVA):
    """the compare executor of (ta, tb): Boolean, never null"""
    if a is None or b is None:
        return op == "!=" and "null_not_equal_is_false" not in rules
    dom = max(ta, tb, key=RANK.get)
    if {ta, tb} == {"FLOAT", "LONG"}:
        if op in ("==", "!="):
            dom = "FLOAT" if "float_long_equal_in_float" in rules else "DOUBLE"
        elif "long_float_order_in_double" in rules:
            dom = "DOUBLE"
    if dom == "FLOAT":
        a, b = _f32(a), _f32(b)
    elif dom == "DOUBLE":
        a, b = float(a), float(b)
    else:
        a, b = int(a), int(b)
    return bool({"==": a == b, "!=": a != b, ">": a > b, ">=": a >= b, "<": a < b, "<=": a <= b}[op])


# ---------------------------------------------------------------------------------------------- expression trees
def var(ref, col):
    return ("var", ref, col)


def const(t, value):
    return ("const", t, value)


def out(k):
    """output column k, inside a `having`"""
    return ("out", k)


def const_text(t, v):
    s = repr(int(v)) if t in ("INT", "LONG") else repr(float(v))
    return s + {"INT": "", "LONG": "L", "FLOAT": "f", "DOUBLE": ""}[t]


def text(e) -> str:
    k = e[0]
    if k == "var":
        return f"{e[1]}.{e[2]}"
    if k == "const":
        return const_text(e[1], e[2])
    if k == "out":
        return f"x{e[1]}"
    if k in ("not", "isnull"):
        return f"not ({text(e[1])})" if k == "not" else f"({text(e[1])}) is null"
    l, r = (text(x) if x[0] in ("var", "const", "out") else f"({text(x)})" for x in e[1:3])
    return f"{l} {k} {r}"


def etype(e, out_types=()) -> str:
    k = e[0]
    if k == "var":
        return COLTYPE[e[2]]
    if k == "const":
        return e[1]
    if k == "out":
        return out_types[e[1]]
    if k in MATH_OPS:
        return max(etype(e[1], out_types), etype(e[2], out_types), key=RANK.get)
    return "BOOL"


def leaves(e, kind="var"):
    if e[0] in ("var", "const", "out"):
        return [e] if e[0] == kind else []
    return [x for sub in e[1:] if isinstance(sub, tuple) for x in leaves(sub, kind)]


def evaluate(e, env, out_types=(), rules=JAVA):
    """value of a tree: env maps (ref, col) -- or an output index -- to a Python scalar or None"""
    k = e[0]
    if k == "var":
        return env[(e[1], e[2])]
    if k == "const":
        return float(np.float32(e[2])) if e[1] == "FLOAT" else e[2]
    if k == "out":
        return env[e[1]]
    if k in MATH_OPS:
        return _jmath(k, evaluate(e[1], env, out_types, rules), evaluate(e[2], env, out_types, rules),
                      etype(e, out_types), rules)
    if k in CMP_OPS:
        return _jcmp(k, evaluate(e[1], env, out_types, rules), etype(e[1], out_types),
                     evaluate(e[2], env, out_types, rules), etype(e[2], out_types), rules)
    if k == "and":
        return evaluate(e[1], env, out_types, rules) is True and evaluate(e[2], env, out_types, rules) is True
    if k == "or":
        return evaluate(e[1], env, out_types, rules) is True or evaluate(e[2], env, out_types, rules) is True
    if k == "not":
        return evaluate(e[1], env, out_types, rules) is not True
    assert k == "isnull", e
    return evaluate(e[1], env, out_types, rules) is None


def right_nested(op, operands):
    e = operands[-1]
    for x in reversed(operands[:-1]):
        e = (op, x, e)
    return e


# ---------------------------------------------------------------------------------------------- bits
def to_bits(v, t) -> int:
    """the C-ABI's 64-bit pattern of an output value (FLOAT: binary32 bits zero-extended)"""
    if t == "FLOAT":
        return int(np.float32(v).view(np.uint32))
    if t == "DOUBLE":
        return int(np.float64(v).view(np.int64))
    return int(v)


def from_bits(bits, t):
    if t == "FLOAT":
        return float(np.uint32(int(bits) & 0xFFFFFFFF).view(np.float32))
    if t == "DOUBLE":
        return float(np.int64(bits).view(np.float64))
    return int(bits)


def is_nan_bits(bits: np.ndarray, t) -> np.ndarray:
    if t == "FLOAT":
        return np.isnan((bits & 0xFFFFFFFF).astype(np.uint32).view(np.float32))
    if t == "DOUBLE":
        return np.isnan(np.ascontiguousarray(bits, np.int64).view(np.float64))
    return np.zeros(len(bits), bool)


def assert_values(got: Outputs, want_vals, want_null, types, what=""):
    """nulls agree; a NaN equals any NaN of the same width; everything else bit for bit, the sign of zero included"""
    assert got.vals.shape == want_vals.shape, (what, got.vals.shape, want_vals.shape)
    gn = got.vnull.astype(bool)
    for k, t in enumerate(types):
        bad = np.flatnonzero(gn[:, k] != want_null[:, k])
        assert not len(bad), f"{what} column {k} ({t}): null differs first at record {bad[0]}"
        g, w = got.vals[:, k], want_vals[:, k]
        if t in ("INT", "FLOAT"):       # 4-byte values: the low word carries them
            g, w = g & 0xFFFFFFFF, w & 0xFFFFFFFF
        same = (g == w) | (is_nan_bits(g, t) & is_nan_bits(w, t)) | want_null[:, k]
        bad = np.flatnonzero(~same)
        assert not len(bad), (f"{what} column {k} ({t}): record {bad[0]} is {from_bits(g[bad[0]], t)!r} "
                              f"({int(g[bad[0]]):#x}), the reference gives {from_bits(w[bad[0]], t)!r} "
                              f"({int(w[bad[0]]):#x})")


def assert_where(got: Outputs, want: Outputs, what=""):
    """trigger, ts, key and group exactly"""
    assert len(got) == len(want), (what, len(got), len(want))
    for f in ("trigger", "ts", "key", "group"):
        x, y = getattr(got, f), getattr(want, f)
        bad = np.flatnonzero(x != y)
        assert not len(bad), f"{what}: field {f} differs first at {bad[0]}: {x[bad[0]]} vs {y[bad[0]]}"


# ---------------------------------------------------------------------------------------------- pools and the pair sweep
F32 = np.float32
POOLS = {
    "INT": [None, 0, 1, -1, 7, -7, 3, 13, 2, -13, 2**24 - 1, 2**24, 2**24 + 1, -2**24 - 1, -2**31, -2**31 + 1, 2**31 - 1,
            2**31 - 2, 46341, -46341, 65536, 100, 1000, -2],
    "LONG": [None, 0, 1, -1, 7, -7, 3, 13, -2, 2**24 + 1, 2**53 + 1, -2**53 - 1, 2**53, -2**63, -2**63 + 1, 2**63 - 1,
             2**63 - 2, 2**60 + 2**36 + 1, 2**40 + 2**16 + 1, 3037000500, -3037000500, 2**31, 2**32, 2**62],
    "FLOAT": [None, 0.0, -0.0, 1.0, -1.0, float(F32(0.1)), -2.5, 7.25, 3.0, 2.0**24 - 1, 2.0**24, 2.0**24 + 2, 2.0**53,
              float(np.finfo(F32).max), -float(np.finfo(F32).max), float(np.finfo(F32).tiny), float(F32(1e-45)),
              -float(F32(1e-45)), np.inf, -np.inf, np.nan, float(F32(1e20)), float(F32(1e-20)), 0.5],
    "DOUBLE": [None, 0.0, -0.0, 1.0, -1.0, 0.1, -2.5, 7.25, 3.0, 16777217.0, 2.0**53, 2.0**53 + 2,
               float(np.finfo(np.float64).max), -float(np.finfo(np.float64).max), float(np.finfo(np.float64).tiny), 5e-324,
               -5e-324, np.inf, -np.inf, np.nan, 1e20, 1e-20, 1e200, 1e-200],
}
NPOOL = 24
VALUE_COLS = (("a", "INT"), ("b", "LONG"), ("f", "FLOAT"), ("d", "DOUBLE"))


def euler_circuit(n):
    """vertices of an Eulerian circuit of the complete directed graph with self-loops on n vertices (Hierholzer):
    n * n + 1 vertices, every ordered pair consecutive exactly once"""
    nxt, stack, walk = [0] * n, [0], []
    while stack:
        u = stack[-1]
        if nxt[u] < n:
            nxt[u] += 1
            stack.append((u + nxt[u]) % n)      # (leave by the other vertices first, the self-loop last)
        else:
            walk.append(stack.pop())
    return walk[::-1]


SEQ = euler_circuit(NPOOL)
N_SWEEP = len(SEQ)                  # 577 rows, 576 consecutive pairs: two 256-thread block edges of the select pass


def pool_columns(index):
    """the four value columns (and their null flags) carrying pool member index[r] in row r"""
    cols, nulls = [], []
    for _, t in VALUE_COLS:
        p = POOLS[t]
        cols.append(np.array([0 if p[i] is None else p[i] for i in index], NP[t]))
        nulls.append(np.array([p[i] is None for i in index], np.uint8))
    return cols, nulls


# ---------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    head: str                       # stream definitions
    pattern: str                    # from ... (up to `select`)
    exprs: list                     # output trees
    rows: str                       # name of the row builder below
    having: Optional[tuple] = None
    partitioned: bool = False
    route: str = ""                 # the route the GPU test expects (ROUTES)
    engine: dict = field(default_factory=dict)
    cuts: List[int] = field(default_factory=list)
    fetch_each: bool = True         # False: one fetch after the last push
    arg: object = None              # the row builder's argument
    floor: int = 1                  # fewest matches of the plain twin

    def __str__(self):
        return self.name

    @property
    def base(self):
        seen = []
        for e in self.exprs:
            for v in leaves(e):
                if v not in seen:
                    seen.append(v)
        return seen

    @property
    def out_types(self):
        return [etype(e) for e in self.exprs]

    def app(self, plain=False) -> str:
        if plain:
            sel = ", ".join(f"{text(v)} as p{k}" for k, v in enumerate(self.base))
        else:
            sel = ", ".join(f"{text(e)} as x{k}" for k, e in enumerate(self.exprs))
            if self.having is not None:
                sel += f" having {text(self.having)}"
        body = f"@info(name='q') from {self.pattern} select {sel} insert into M;"
        if self.partitioned:
            stream = self.head.split("define stream ")[1].split(" ")[0]
            body = f"partition with (symbol of {stream}) begin {body} end;"
        return self.head + " " + body


HEAD_S = "define stream S (id long, symbol string, a int, b long, f float, d double);"
EVERY = "every e1=S -> e2=S[id > e1.id] within 10 sec"
ONCE = "e1=S -> e2=S[id > e1.id]"
E1 = {c: var("e1", c) for c, _ in VALUE_COLS}
E2 = {c: var("e2", c) for c, _ in VALUE_COLS}
COL_OF = {t: c for c, t in VALUE_COLS}


def _batch(n, ts, stream, key, cols, nulls):
    return Batch(n, 0, np.asarray(ts, np.int64), np.asarray(stream, np.int32), np.asarray(key, np.int32), cols,
                 [x if x is not None and x.any() else None for x in nulls])


def rows_sweep(_):
    """row r carries pool member SEQ[r] in all four value columns; id = r, one key"""
    n = N_SWEEP
    cols, nulls = pool_columns(SEQ)
    return _batch(n, T0 + np.arange(n), np.zeros(n), np.zeros(n),
                  [np.arange(n, dtype=np.int64), np.zeros(n, np.int32)] + cols, [None, None] + nulls)


def rows_once(_):
    """every ordered pool pair its own key of two rows"""
    index = [i for p in range(N_SWEEP - 1) for i in (SEQ[p], SEQ[p + 1])]
    n = len(index)
    key = np.arange(n, dtype=np.int32) // 2
    cols, nulls = pool_columns(index)
    return _batch(n, T0 + np.arange(n), np.zeros(n), key, [np.arange(n, dtype=np.int64), key.copy()] + cols,
                  [None, None] + nulls)


HEAD_C4 = ("@app:playback define stream S (id long, seq long, a int, b long, f float, d double); "
           "define stream Tick (x int);")
N_ABSENT, ABSENT_KILLED = 600, 80


def rows_absent(_):
    """C4's stream with the value columns: ids 0 .. 519, then 80 rows that repeat the first ids inside their 5 s (those
    e1 are killed); a closing Tick row fires every timer left"""
    n = N_ABSENT + 1
    ids = np.arange(n, dtype=np.int64)
    ids[N_ABSENT - ABSENT_KILLED:N_ABSENT] -= N_ABSENT - ABSENT_KILLED
    ts = T0 + 5 * np.arange(n, dtype=np.int64)
    ts[-1] = ts[-2] + 5001
    stream = np.zeros(n, np.int32)
    stream[-1] = 1
    cols, nulls = pool_columns([(r + r // NPOOL) % NPOOL for r in range(n)])
    return _batch(n, ts, stream, np.zeros(n), [ids, np.arange(n, dtype=np.int64)] + cols + [np.zeros(n, np.int32)],
                  [None, None] + nulls + [None])


HEAD_C3 = "define stream S (id long, symbol string, v int, w int, a int, b long, f float, d double);"
N_LANES, KEYS_LANES = 20_000, 50


def rows_lanes(cfg):
    """the rows of synth config C3b / C3c (the filters read v / w) widened by the four value columns"""
    n = N_LANES
    g = synth.generate(cfg, 0, n, keys=KEYS_LANES, rate=1000)
    uniq, first = np.unique(g["key"], return_index=True)        # dense ids in first-seen order
    rank = np.empty(len(uniq), np.int32)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq), dtype=np.int32)
    key = rank[np.searchsorted(uniq, g["key"])]
    cols, nulls = pool_columns([(r * 7 + r // NPOOL) % NPOOL for r in range(n)])
    return _batch(n, g["ts"], np.zeros(n), key, [g["id"], g["key"].astype(np.int32), g["v"], g["w"]] + cols,
                  [None] * 4 + nulls)


HEAD_C = "define stream S (id long, symbol string, v int, flag int);"
KEEP_PATTERNS = ("none", "all", "first", "last", "alternate", "255_256")


def keep_flags(n, pattern):
    f = np.zeros(n, np.int32)
    if pattern == "all":
        f[:] = 1
    elif pattern == "first":
        f[0] = 1
    elif pattern == "last":
        f[n - 1] = 1
    elif pattern == "alternate":
        f[::2] = 1
    elif pattern == "255_256":
        f[255:257] = 1
    return f


def rows_compact(flags):
    """len(flags) matches: record r is (row r, row r + 1) and carries flags[r]"""
    n = len(flags) + 1
    r = np.arange(n, dtype=np.int64)
    return _batch(n, T0 + r, np.zeros(n), np.zeros(n),
                  [r, np.zeros(n, np.int32), ((r * 37) % 1000).astype(np.int32), np.append(flags, 0).astype(np.int32)],
                  [None] * 4)


HEAD_W = "define stream S (" + ", ".join(f"c{k} int" for k in range(16)) + ");"
N_WIDE = 300


def rows_wide(_):
    """16 INT columns: c0 = row number, the others tame, c15 null on every third row"""
    n = N_WIDE
    r = np.arange(n, dtype=np.int64)
    cols = [r.astype(np.int32)] + [((r * (k + 3) + k * k) % 1000 - 500).astype(np.int32) for k in range(1, 16)]
    return _batch(n, T0 + r, np.zeros(n), np.zeros(n), cols, [None] * 15 + [(r % 3 == 0).astype(np.uint8)])


ROWS = {"sweep": rows_sweep, "once": rows_once, "absent": rows_absent, "lanes": rows_lanes, "compact": rows_compact,
        "wide": rows_wide}
_BATCHES = {}


def batch(case: Case) -> Batch:
    """the case's whole stream (made once per row set, never changed)"""
    k = (case.rows, case.arg if not isinstance(case.arg, np.ndarray) else case.arg.tobytes())
    if k not in _BATCHES:
        _BATCHES[k] = ROWS[case.rows](case.arg)
    return _BATCHES[k]


def pushes(case: Case) -> List[Batch]:
    b, out_, lo = batch(case), [], 0
    for hi in list(case.cuts) + [b.n]:
        out_.append(Batch(hi - lo, lo, b.ts[lo:hi], b.stream[lo:hi], b.key[lo:hi],
                          [np.ascontiguousarray(c[lo:hi]) for c in b.cols],
                          [None if x is None else np.ascontiguousarray(x[lo:hi]) for x in b.nulls]))
        lo = hi
    return out_


# ---- expression groups of the pair sweep
def pair_group(lt):
    """`e1.<lt column> op e2.<column>` for every right type and operator"""
    return [(op, E1[COL_OF[lt]], E2[COL_OF[rt]]) for rt in TYPES for op in MATH_OPS]


I, LG, FL, DB = "INT", "LONG", "FLOAT", "DOUBLE"
CONSTANTS = [
    ("/", E1["a"], const(I, 0)), ("/", E1["f"], const(I, 0)), ("%", E1["d"], const(DB, -0.0)),
    ("%", E1["b"], const(LG, 0)),
    ("*", E2["b"], const(LG, 2)), ("+", E1["a"], const(FL, 0.1)), ("+", E1["a"], const(DB, 0.1)),
    ("/", const(I, 7), E2["a"]), ("%", const(LG, 5), E2["b"]), ("-", const(FL, 1.5), E2["f"]),
    ("/", const(DB, 1.5), E2["d"]),
    ("+", E1["b"], const(I, 1)), ("*", E1["f"], const(LG, 2)), ("-", const(I, 100), E1["b"]),
    ("+", E2["d"], const(FL, 1.5)),
    ("+", const(I, 16777217), E1["f"]), ("+", const(LG, 2**63 - 1), E2["a"]), ("/", E1["b"], const(I, -1)),
    ("%", E1["a"], const(I, -1)), ("/", E1["a"], const(I, -1)), ("*", E1["d"], const(LG, 2**53 + 1)),
    ("%", E2["f"], const(FL, 0.1)), ("/", const(LG, 2**60 + 2**36 + 1), E2["f"]),
]
NESTED = [
    ("*", ("+", E1["b"], E2["a"]), E2["f"]), ("+", ("*", E1["f"], E2["f"]), E2["d"]), ("/",
    ("*", E1["a"], E2["a"]), E2["b"]),
    ("+", ("+", E1["a"], E2["a"]), E2["b"]), ("%", ("*", E1["b"], E2["b"]), E2["a"]), ("-", E1["d"],
    ("/", E1["f"], E2["f"])),
    ("*", ("/", E1["a"], E2["a"]), const(FL, 1.5)), ("-", ("*", ("+", E1["a"], E2["a"]), E2["a"]), E1["b"]),
    ("-", ("+", E1["f"], E2["b"]), E2["b"]), ("+", ("%", E1["b"], E2["a"]), ("%", E1["f"], E2["f"])),
    ("/", ("-", E1["b"], E2["b"]), ("*", E1["d"], E2["f"])),
]
GROUPS = {**{f"pairs-{t}": pair_group(t) for t in TYPES}, "constants": CONSTANTS, "nested": NESTED}

# the sweep's routes: (pattern, partitioned, GpuEngine keywords)
SWEEP_ROUTES = {
    "tiled": (EVERY, True, {}),
    "search": (EVERY, False, {}),
    "flat_walker": (EVERY, False, {"walker_only": True}),
    # the general family takes `every e1 -> e2 within T` on its partial lanes unless told otherwise
    "lanes": (EVERY, False, {"force_general": True}),
    "machine": (EVERY, False, {"force_general": True, "partial_lanes": -1}),
}


def sweep_case(name, exprs, route="search", having=None, **kw):
    pattern, partitioned, engine = SWEEP_ROUTES[route]
    return Case(name, HEAD_S, pattern, exprs, "sweep", having=having, partitioned=partitioned, route=route,
                engine=dict(engine), floor=N_SWEEP - 1, **kw)


def group_cases() -> List[Case]:
    out_ = [sweep_case(f"{g}-{route}", exprs, route) for g, exprs in GROUPS.items() for route in SWEEP_ROUTES]
    out_ += [Case(f"{g}-once", HEAD_S, ONCE, exprs, "once", partitioned=True, route="once", floor=N_SWEEP - 1)
             for g, exprs in GROUPS.items()]
    return out_


# ---- having: one select list, one condition per case
HSEL = [("+", E1["a"], E2["a"]), ("-", E1["b"], E2["b"]), ("*", E1["f"], E2["f"]), ("/", E1["d"], E2["d"]),
        E2["a"], E1["b"], E2["f"], E2["d"], E1["f"], ("/", E1["a"], E2["a"]), E2["b"]]
X = [out(k) for k in range(len(HSEL))]
HAVING = {**{f"i64-{op}": (op, X[0], X[4]) for op in CMP_OPS},
          **{f"f32-{op}": (op, X[2], X[6]) for op in CMP_OPS},
          **{f"f64-{op}": (op, X[3], X[7]) for op in CMP_OPS},
          "long==float": ("==", X[5], X[6]), "long>float": (">", X[5], X[6]), "float<=long": ("<=", X[8], X[10]),
          "nan-==": ("==", X[2], X[2]), "nan-!=": ("!=", X[2], X[2]), "nan->=": (">=", X[2], X[2]),
          "nan-<=": ("<=", X[2], X[2]), "nan-<>": ("or", ("or", (">", X[2], X[2]), ("<", X[2], X[2])),
          (">", X[0], const(I, 0))),
          "zero-==": ("==", X[8], const(DB, 0.0)),
          "null-!=": ("!=", X[9], const(I, 1)), "null-not": ("not", (">", X[9], const(I, 1))),
          "null-isnull": ("isnull", X[9]),
          "mix": ("or", ("and", (">", X[0], const(I, 0)), ("not", ("isnull", X[2]))), ("==", X[9], const(I, 0)))}


def having_cases() -> List[Case]:
    return [sweep_case(f"having-{k}", HSEL, "search", having=h) for k, h in HAVING.items()]


# ---- compaction behind `having`
CSEL = [var("e1", "id"), var("e2", "id"), var("e1", "flag"), ("+", var("e1", "v"), var("e2", "v"))]
COMPACT_N = (1, 255, 256, 257, 512, 513)


def compact_cases() -> List[Case]:
    hv = ("==", out(2), const(I, 1))
    out_ = []
    for n in COMPACT_N:
        for p in KEEP_PATTERNS:
            if p == "255_256" and n < 257:
                continue
            out_.append(Case(f"compact-{n}-{p}", HEAD_C, EVERY, CSEL, "compact", having=hv, route="search",
                             arg=keep_flags(n, p), floor=n))
    # two pushes, one fetch after the second: the second push's kept records append behind the first's
    some, none = keep_flags(300, "alternate"), keep_flags(300, "none")
    for name, flags in (("some_then_none", np.append(some, none)), ("none_then_some", np.append(none, some))):
        out_.append(Case(f"compact-two_pushes-{name}", HEAD_C, EVERY, CSEL, "compact", having=hv, route="search",
                         arg=flags, cuts=[300], fetch_each=False, floor=600))
    return out_


# ---- 32 outputs over 32 base slots
def wide_case() -> Case:
    e1, e2 = [var("e1", f"c{k}") for k in range(16)], [var("e2", f"c{k}") for k in range(16)]
    # (base slots in first-use order: e1.c0, e2.c0 .. e1.c15, e2.c15: slots 30, 31 and outputs 15, 31 see c15's nulls)
    exprs = [("+", e1[k], e2[k]) for k in range(16)] + [("-", e2[15 - k], e1[k]) for k in range(16)]
    return Case("wide-32", HEAD_W, "every e1=S -> e2=S[c0 > e1.c0] within 10 sec", exprs, "wide", route="search",
                floor=N_WIDE - 1)


# ---- programs of exactly the VM's depth
VM_DEPTH = 16


def int_sum(k, leaf=lambda j: (E1 if j % 2 == 0 else E2)["a"]):
    return right_nested("+", [leaf(j) for j in range(k)])


def deep_filter(k):
    """a right-nested filter of k compares over the row's own columns: operand stack k + 1"""
    cmps = [(">", "a", "0"), ("<=", "b", "7L"), ("!=", "f", "1.0f"), (">=", "d", "-2.5"), ("<", "a", "65536"), ("==",
    "b", "1L")]
    parts = [f"{c} {op} {x}" for op, c, x in (cmps[j % 6] for j in range(k))]
    e = parts[-1]
    for j in range(k - 2, -1, -1):
        e = f"{parts[j]} {'and' if j % 2 == 0 else 'or'} ({e})"
    return e


def deep_filter_pattern(k):
    return f"every e1=S -> e2=S[{deep_filter(k)}]"


def depth_cases(k=VM_DEPTH) -> List[Case]:
    """a right-nested k-operand INT sum (its partial sums wrap) as a select output and inside a `having`, and a
    right-nested filter of stack depth k on the per-key machine"""
    ids = [var("e1", "id"), var("e2", "id")]
    return [
        sweep_case(f"depth{k}-select", [int_sum(k), E1["a"], E2["a"]]),
        sweep_case(f"depth{k}-having", [E1["a"], E2["a"]], having=(">", int_sum(k, lambda j: out(j % 2)), const(I, 0))),
        Case(f"depth{k}-filter", HEAD_S, deep_filter_pattern(k - 1), ids + [("+", E1["a"], E2["a"])], "sweep",
             route="machine", engine={"force_general": True, "partial_lanes": -1}, floor=200),
    ]


# ---- the other routes
def _pattern_of(cfg):
    q = synth.QUERIES[cfg]
    return q[q.index("from ") + 5:q.index(" select")]


def _lane_exprs():
    e1 = {c: var("e1", c) for c in "abfd"}
    z = {c: var("e2[last]", c) for c in "abfd"}
    return [var("e1", "id"), ("-", z["f"], var("e2[0]", "f")), ("+", var("e3", "a"), const(I, 1)),
            ("*", var("e4", "b"), const(LG, 2)), ("/", e1["d"], z["d"]), ("%", e1["a"], z["a"]), ("+", e1["b"], e1["f"]),
            ("/", ("*", e1["a"], z["a"]), e1["b"]), ("*", e1["f"], var("e2[0]", "f")), ("-", var("e3", "d"), var("e4",
            "f")),
            ("/", e1["b"], z["a"])]


def route_cases() -> List[Case]:
    own = [(op, E1[COL_OF[lt]], E1[COL_OF[rt]]) for lt, rt, op in
           ((I, LG, "+"), (FL, DB, "*"), (LG, I, "/"), (FL, I, "%"), (DB, LG, "-"), (LG, FL, "+"), (I, I, "*"),
           (DB, FL, "/"),
            (LG, LG, "%"), (FL, FL, "-"))]
    return [
        Case("absent", HEAD_C4, "every e1=S -> not S[id==e1.id] for 5 sec", [var("e1", "seq")] + own, "absent",
             route="absent", floor=200),
        Case("sequence_lanes", HEAD_C3, _pattern_of("C3b"), _lane_exprs(), "lanes", arg="C3b", partitioned=True,
             route="sequence_lanes", floor=200),
        Case("partial_lanes", HEAD_C3, _pattern_of("C3c"), _lane_exprs(), "lanes", arg="C3c", partitioned=True,
             route="partial_lanes", floor=200),
    ]


GROUP_CASES, HAVING_CASES, COMPACT_CASES = group_cases(), having_cases(), compact_cases()
WIDE, DEPTH_CASES, ROUTE_CASES = wide_case(), depth_cases(), route_cases()
ALL = GROUP_CASES + HAVING_CASES + COMPACT_CASES + [WIDE] + DEPTH_CASES + ROUTE_CASES
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)

# kernel names (sg_timing) that tell the routes apart: (some of these ran, none of these ran)
ROUTES = {
    "tiled": (("walk_count",), ("nge_search", "group_walk", "nfa_keys", "nfa_units")),
    "search": (("nge_search",), ("walk_count", "nfa_keys", "nfa_units")),
    "flat_walker": (("walk_count",), ("nge_search", "nfa_keys", "nfa_units")),
    "lanes": (("partial_lanes",), ("walk_count", "nge_search", "nfa_keys", "nfa_units")),
    "machine": (("nfa_keys", "nfa_units"), ("walk_count", "nge_search", "sequence_lanes", "partial_lanes")),
    "once": (("once_match",), ("nfa_keys", "nfa_units")),
    "absent": (("abs_roles",), ("abs_sequential", "nfa_keys", "nfa_units")),
    "sequence_lanes": (("sequence_lanes",), ("nfa_keys",)),
    "partial_lanes": (("partial_lanes",), ("nfa_keys", "nfa_units")),
}


# ---------------------------------------------------------------------------------------------- running
def run(engine_factory, app, batches, fetch_each=True) -> Outputs:
    from parity_util import context
    ctx = context(app)
    eng = engine_factory(ctx)
    outs = []
    for k, b in enumerate(batches):
        eng.push(b)
        if fetch_each or k == len(batches) - 1:
            outs.append(eng.fetch())
    eng.close()
    return Outputs(*[np.concatenate([getattr(o, f) for o in outs]) for f in
                     ("trigger", "ts", "key", "group", "vals", "vnull")])


def oracle(case: Case, plain=False) -> Outputs:
    from oracle import OracleEngine
    return run(OracleEngine, case.app(plain), pushes(case), case.fetch_each)


@lru_cache(maxsize=None)
def _plain(name) -> Outputs:
    return oracle(BY_NAME[name], plain=True)


def base_values(case: Case):
    """per record of the plain twin: {(ref, col): value} of the matched base slots, from the oracle"""
    o = _plain(case.name)
    base = case.base
    types = [COLTYPE[c] for _, _, c in base]
    return [{(v[1], v[2]): None if o.vnull[r, k] else from_bits(o.vals[r, k], types[k]) for k, v in enumerate(base)}
            for r in range(len(o))]


def reference(case: Case, rules=JAVA):
    """(where, vals, null): the plain twin's trigger / ts / key / group of the records that pass `having`, and the
    reference's output values as bit patterns"""
    o = _plain(case.name)
    types = case.out_types
    vals, null, keep = [], [], []
    for env in base_values(case):
        row = [evaluate(e, env, rules=rules) for e in case.exprs]
        if case.having is not None and evaluate(case.having, dict(enumerate(row)), types, rules) is not True:
            keep.append(False)
            continue
        keep.append(True)
        vals.append([0 if x is None else to_bits(x, t) for x, t in zip(row, types)])
        null.append([x is None for x in row])
    keep = np.array(keep, bool)
    where = Outputs(o.trigger[keep], o.ts[keep], o.key[keep], o.group[keep], None, None)
    return (where, np.array(vals, np.int64).reshape(-1, len(types)), np.array(null, bool).reshape(-1, len(types)))


@lru_cache(maxsize=None)
def expected(name):
    return reference(BY_NAME[name])


def check(case: Case, got: Outputs, what):
    """an engine's output on the expression twin against the reference (values) and the plain twin (where)"""
    where, vals, null = expected(case.name)
    assert len(got) == len(vals), (what, case.name, len(got), len(vals))
    assert_where(got, where, f"{what} {case.name}")
    assert_values(got, vals, null, case.out_types, f"{what} {case.name}")


def run_gpu(case: Case):
    """(output, kernel names per push) of the HIP engine over the case's expression twin"""
    from siddhi_amd._native import GpuEngine
    log = []

    class Witness(GpuEngine):
        def __init__(self, ctx):
            super().__init__(ctx, **case.engine)

        def push(self, b):
            super().push(b)
            log.append([name for name, _ in self.handle.timing().kernels()])

    return run(Witness, case.app(), pushes(case), case.fetch_each), log


def check_route(case: Case, log):
    some, none = ROUTES[case.route]
    names = [n for push in log for n in push]
    assert any(n in names for n in some) and not any(n in names for n in none), f"{case.name} ({case.route}): {log}"
