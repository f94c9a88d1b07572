"""Cases of the aggregate tests (test_agg_cases.py on the CPU, test_agg_gpu.py on the GPU).

Expected output of a case: the oracle runs the case's BASE app -- the same pattern selecting the group-by attributes
and the aggregators' arguments as plain columns -- and agg_ref.fold folds those ordered records.  No pattern rule is
restated here (the device select_ref.py uses)."""
import struct
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Tuple

import numpy as np

import agg_ref as R
from siddhi_amd.runtime import Batch, Outputs

STREAM = ("define stream S (id long, symbol string, p int, iv int, lv long, fv float, dv double, gi int, gf float, "
          "gl long, gs string);")
COLS = ["id", "symbol", "p", "iv", "lv", "fv", "dv", "gi", "gf", "gl", "gs"]
TYPES = dict(id="LONG", symbol="STRING", p="INT", iv="INT", lv="LONG", fv="FLOAT", dv="DOUBLE", gi="INT", gf="FLOAT",
             gl="LONG", gs="STRING")
NP = {"STRING": np.int32, "INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64}
PATTERN = "from every e1=S[p>20] -> e2=S[p > e1.p] within 1 sec"

I32_MAX, I64_MAX = 2**31 - 1, 2**63 - 1
F32_DENORM = struct.unpack("<f", struct.pack("<I", 1))[0]
POOLS = {
    # integer extremes (sum wraps), 2^53 +- 1 (avg leaves the exact range)
    "iv": [0, 1, -1, 7, I32_MAX, -I32_MAX - 1, I32_MAX - 1, 1000],
    "lv": [0, 1, -1, I64_MAX, -I64_MAX - 1, 2**53, 2**53 + 1, 2**53 - 1, -(2**53), 12345],
    # 1e16 / 1.0 / -1e16 runs (a reordered sum changes bits), NaN, both zeros, denormals
    "fv": [1e16, 1.0, -1e16, 0.0, -0.0, float("nan"), F32_DENORM, -F32_DENORM, 3.5, 16777216.0, 0.1],
    "dv": [1e16, 1.0, -1e16, 0.0, -0.0, float("nan"), 5e-324, -5e-324, 2.5, 0.1, 1e308],
    "gi": [0, 1, -1, 5],
    "gf": [0.0, -0.0, float("nan"), 1.5, -1.5],
    "gl": [0, 2**40, -(2**40), 9],
    "gs": [0, 1, 2],
}


@dataclass
class Case:
    name: str
    aggs: List[Tuple[str, Optional[str], str]]           # (aggregator, argument expression or None, argument TYPE)
    groups: List[Tuple[str, str]] = field(default_factory=list)     # (attribute reference, TYPE)
    part: bool = True
    having: Optional[Tuple[str, Callable]] = None        # (SiddhiQL over a0.., the same over the list of values)
    n: int = 1500
    keys: int = 6
    seed: int = 1
    cuts: Optional[List[int]] = None                     # push boundaries (rows); None: one push
    pattern: str = PATTERN
    null_frac: float = 0.03
    pools: dict = field(default_factory=dict)            # column -> pool replacing POOLS[column]
    head_null: bool = False                              # key 0's first arguments all null
    engine_kw: dict = field(default_factory=dict)
    ts_step: int = 1                                     # ms between rows
    app_head: str = ""                                   # app annotations (@app:playback)

    def __str__(self):
        return self.name

    # ---- apps
    def _wrap(self, body):
        if self.part:
            return f"{self.app_head}{STREAM} partition with (symbol of S) begin @info(name='q') {body} end;"
        return f"{self.app_head}{STREAM} @info(name='q') {body}"

    def agg_app(self):
        sel = [f"{g} as g{k}" for k, (g, _) in enumerate(self.groups)]
        sel += [f"{n}({a or ''}) as a{k}" for k, (n, a, _) in enumerate(self.aggs)]
        gb = (" group by " + ", ".join(g for g, _ in self.groups)) if self.groups else ""
        hv = f" having {self.having[0]}" if self.having else ""
        return self._wrap(f"{self.pattern} select {', '.join(sel)}{gb}{hv} insert into M;")

    def base_app(self):
        sel = [f"{g} as g{k}" for k, (g, _) in enumerate(self.groups)]
        sel += [f"{a} as x{k}" for k, (_, a, _) in enumerate(self.aggs) if a is not None]
        sel += ["e1.id as i1"]     # (a select list is never empty)
        return self._wrap(f"{self.pattern} select {', '.join(sel)} insert into M;")

    # ---- rows
    def batches(self):
        rng = np.random.default_rng(self.seed)
        n = self.n
        cols, nulls = {}, {}
        cols["id"] = np.arange(n, dtype=np.int64)
        cols["symbol"] = rng.integers(0, self.keys, n).astype(np.int32)
        cols["p"] = rng.integers(15, 60, n).astype(np.int32)
        for c in ("iv", "lv", "fv", "dv", "gi", "gf", "gl", "gs"):
            pool = np.array(self.pools.get(c, POOLS[c]), dtype=NP[TYPES[c]])
            cols[c] = pool[rng.integers(0, len(pool), n)]
            nul = (rng.random(n) < self.null_frac).astype(np.uint8)
            if self.head_null and c in ("iv", "lv", "fv", "dv"):
                first = np.nonzero(cols["symbol"] == cols["symbol"][0])[0][:40]
                nul[first] = 1
            nulls[c] = nul
        ts = 1000 + self.ts_step * np.arange(n, dtype=np.int64)
        key = _dense(cols["symbol"]) if self.part else np.zeros(n, np.int32)
        cl = [cols[c] for c in COLS]
        nl = [nulls.get(c) for c in COLS]
        cuts = [0] + list(self.cuts or []) + [n]
        out = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            out.append(Batch(hi - lo, lo, ts[lo:hi], np.zeros(hi - lo, np.int32), key[lo:hi], [c[lo:hi] for c in cl],
                             [None if x is None else x[lo:hi] for x in nl]))
        return out


def _dense(keys):
    uniq, first = np.unique(keys, return_index=True)
    order = np.argsort(first, kind="stable")
    ids = np.empty(len(uniq), np.int32)
    ids[order] = np.arange(len(uniq), dtype=np.int32)
    return ids[np.searchsorted(uniq, keys)]


def run_pushes(engine_factory, app, batches):
    """per push Outputs of `app` on the engine"""
    from parity_util import context
    eng = engine_factory(context(app))
    outs = []
    try:
        for b in batches:
            if b.n:
                eng.push(b)
            outs.append(eng.fetch())
    finally:
        eng.close()
    return outs


_BASE = {}


def base_outputs(case: Case):
    """the oracle's outputs of the base app, per push (computed once per case and left unchanged)"""
    if case.name not in _BASE:
        from oracle import OracleEngine
        _BASE[case.name] = run_pushes(OracleEngine, case.base_app(), case.batches())
    return _BASE[case.name]


def _val(o: Outputs, i, k, t):
    if o.vnull[i, k]:
        return None
    v = R.from_bits(o.vals[i, k], t)
    return v


def records(case: Case, base):
    """agg_ref records of the base outputs, per push"""
    ng = len(case.groups)
    pushes = []
    for o in base:
        recs = []
        for i in range(len(o)):
            gv = [_val(o, i, k, t) for k, (_, t) in enumerate(case.groups)]
            args, x = [], ng
            for (_, a, t) in case.aggs:
                if a is None:
                    args.append(0)
                else:
                    args.append(_val(o, i, x, t))
                    x += 1
            recs.append((int(o.key[i]), gv, args))
        pushes.append(recs)
    return pushes


def expected(case: Case, wrong=None):
    """per push: (the base Outputs, [(record index, [aggregate values])]) after `having`"""
    base = base_outputs(case)
    rows = R.fold(records(case, base), [(n, t) for n, _, t in case.aggs], [t for _, t in case.groups], case.part,
                  case.having[1] if case.having else None, wrong)
    return base, rows


def check(case: Case, got, where=""):
    """got: per push Outputs of the aggregate app"""
    base, rows = expected(case)
    ng = len(case.groups)
    rtypes = [R.result_type(n, t) for n, _, t in case.aggs]
    assert len(got) == len(base)
    for p, (g, b, rw) in enumerate(zip(got, base, rows)):
        assert len(g) == len(rw), f"{where}{case.name} push {p}: {len(g)} matches, expected {len(rw)}"
        ix = np.array([i for i, _ in rw], dtype=np.int64)
        for f in ("trigger", "ts", "key", "group"):
            assert np.array_equal(getattr(g, f), getattr(b, f)[ix]), f"{where}{case.name} push {p}: {f} differs"
        for j, (i, vals) in enumerate(rw):
            for k in range(ng):     # the plain columns in front
                assert g.vnull[j, k] == b.vnull[i, k] and (b.vnull[i, k] or g.vals[j, k] == b.vals[i, k]), \
                    f"{where}{case.name} push {p} match {j}: group column {k}"
            for k, (want, t) in enumerate(zip(vals, rtypes)):
                gn, gb = bool(g.vnull[j, ng + k]), g.vals[j, ng + k]
                assert gn == (want is None), \
                    f"{where}{case.name} push {p} match {j} {case.aggs[k][0]}: null {gn}, expected {want!r}"
                if want is not None:
                    assert R.same_value(gb, want, t), (f"{where}{case.name} push {p} match {j} {case.aggs[k]}: got "
                                                       f"{R.from_bits(gb, t)!r} ({int(gb):#x}), expected {want!r}")


# ---------------------------------------------------------------------------------------------------- the cases
def _cuts3(n):
    return [1, n // 2, n // 2 + 1]


ARG = {"INT": "e2.iv", "LONG": "e2.lv", "FLOAT": "e2.fv", "DOUBLE": "e2.dv"}

# every aggregator x argument type, one push and three pushes
TYPE_CASES = []
for _t in ("INT", "LONG", "FLOAT", "DOUBLE"):
    _aggs = [("count", ARG[_t], _t), ("sum", ARG[_t], _t), ("avg", ARG[_t], _t), ("min", ARG[_t], _t),
             ("max", ARG[_t], _t)]
    TYPE_CASES.append(Case(f"types-{_t}-1push", _aggs, seed=11))
    TYPE_CASES.append(Case(f"types-{_t}-3push", _aggs, cuts=_cuts3(1500), seed=12, head_null=True))

ALL5 = [("count", None, "INT"), ("sum", "e2.iv", "INT"), ("avg", "e2.dv - e1.dv", "DOUBLE"), ("max", "e2.fv", "FLOAT"),
        ("min", "e2.dv", "DOUBLE")]

GROUP_CASES = [
    Case("nogroup-part", ALL5, cuts=_cuts3(1500)),
    Case("nogroup-unpart", ALL5, part=False, cuts=_cuts3(1500)),
    Case("group-string", ALL5, [("e1.gs", "STRING")], cuts=_cuts3(1500)),
    Case("group-int-unpart", ALL5, [("e1.gi", "INT")], part=False, cuts=_cuts3(1500)),
    Case("group-float", ALL5, [("e2.gf", "FLOAT")], cuts=_cuts3(1500), null_frac=0.08),
    Case("group-float-long", ALL5, [("e1.gf", "FLOAT"), ("e2.gl", "LONG")], cuts=_cuts3(1500)),
    Case("group-four", ALL5, [("e1.gs", "STRING"), ("e2.gi", "INT"), ("e1.gf", "FLOAT"), ("e2.gl", "LONG")],
         cuts=_cuts3(1500)),
]

HAVING_CASES = [
    Case("having-count", ALL5, [("e1.gs", "STRING")], having=("a0 > 3", lambda v: v[0] > 3), cuts=_cuts3(1500)),
    # every match of the second push is dropped (the running count passes 95 with the first push's last match and 771
    # with the second's; test_agg_cases.py checks that on the oracle's counts); the third push shows the state the
    # second left
    Case("having-drops-a-push", [("count", None, "INT"), ("sum", "e2.iv", "INT")], part=False,
         having=("a0 <= 95 or a0 > 771", lambda v: v[0] <= 95 or v[0] > 771), pools={"iv": [1, 2, 3]},
         cuts=[120, 900]),
]

# avg over LONG with partial sums crossing 2^53: the serial fallback
AVG53 = Case("avg-long-2p53", [("avg", "e2.lv", "LONG"), ("count", None, "INT")], [("e1.gi", "INT")],
             pools={"lv": [2**52, 2**52 + 1, 3, -5, 2**51]}, cuts=_cuts3(1500))
AVG_EXACT = Case("avg-long-exact", [("avg", "e2.lv", "LONG"), ("avg", "e2.iv", "INT")], [("e1.gi", "INT")],
                 pools={"lv": [2**40, -(2**40), 3, -5, 2**31], "iv": [I32_MAX, -I32_MAX - 1, 5]}, cuts=_cuts3(1500))

ALL = TYPE_CASES + GROUP_CASES + HAVING_CASES + [AVG53, AVG_EXACT]
