"""The device range router (sg_range_*, siddhi_amd/csrc/ranges.hip) against the host router.

Range routing had one implementation (runtime._range_mask / _range_route) under both the oracle and the GPU engine.
The device router is a second one: lowering.lower_ranges turns every range condition into a postfix program, the hold
kernel evaluates the programs per row and the expand kernel writes one copy per holding range.  The CPU tests pin the
programs against the host masks with a numpy interpreter of the postfix code written here, the FLOAT/LONG equality rule
against a hand-derived value, and the ABI's struct layout against C.  The GPU tests compare the routed device batch
with _range_route over _range_mask field by field, and with rows written out by hand, then run whole apps through
send_columns on both routes.  Both routers share lowering._cmp_domain, so a second group of GPU tests takes its
expected values from range_ref.py, a row-at-a-time restatement that shares no code with either: every type and compare
domain on edge values, every instantiation of the hold kernel, first holders in other waves and tiles than the first,
and the optional arrays of the batch left out."""
import ctypes as ct
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))

import range_cases as RC  # noqa: E402
import range_ref  # noqa: E402
from oracle import OracleEngine  # noqa: E402  (checker engine; CPU)
from siddhi_amd import QueryCallback, SiddhiManager  # noqa: E402
from siddhi_amd import compiler as C  # noqa: E402
from siddhi_amd import lowering as L  # noqa: E402
from siddhi_amd.runtime import Batch, _range_mask  # noqa: E402
from test_range_partition import ABSENT_APP, RANGES, _random_rows, app  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "siddhi_gpu.h")
NP = {"STRING": np.int32, "INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64,
      "BOOL": np.int32}
TYPE_OF_CODE = {v: k for k, v in L.TYPE_CODE.items()}


# ------------------------------------------------------------------------------------------- CPU: programs
def interpret(prog, cols, nulls, n):
    """numpy interpreter of a postfix range program: bool[n].  Stack entries are (values, type, null mask); the rules
    are the executors' (a compare with a null operand is false, != true; and / or / not read null as false)."""
    st, pc = [], 0
    no = np.zeros(n, bool)

    def truth(x):
        return (x[0] != 0) & ~x[2]

    while pc < len(prog):
        op = prog[pc]
        if op == L.OP_VAR:
            col, t = prog[pc + 3], TYPE_OF_CODE[prog[pc + 4]]
            st.append((cols[col], t, no if nulls[col] is None else nulls[col].astype(bool)))
            pc += 5
        elif op == L.OP_CONST:
            t, bits = TYPE_OF_CODE[prog[pc + 1]], prog[pc + 2]
            if t == "FLOAT":
                v = np.float32(struct.unpack("<f", struct.pack("<I", bits))[0])
            elif t == "DOUBLE":
                v = struct.unpack("<d", struct.pack("<q", bits))[0]
            else:
                v = bits
            st.append((np.full(n, v, NP[t] if t not in ("STRING", "BOOL") else np.int64), t, no))
            pc += 3
        elif op == L.OP_CMP:
            r, l_ = st.pop(), st.pop()
            dt = {L.D_F32: np.float32, L.D_F64: np.float64}.get(prog[pc + 2], np.int64)
            f = [np.equal, np.not_equal, np.greater, np.greater_equal, np.less, np.less_equal][prog[pc + 1]]
            v = f(l_[0].astype(dt), r[0].astype(dt))
            anynull = l_[2] | r[2]
            st.append(((v | anynull) if prog[pc + 1] == 1 else (v & ~anynull), "BOOL", no))
            pc += 3
        elif op in (L.OP_AND, L.OP_OR):
            r, l_ = st.pop(), st.pop()
            st.append(((truth(l_) & truth(r)) if op == L.OP_AND else (truth(l_) | truth(r)), "BOOL", no))
            pc += 1
        elif op == L.OP_NOT:
            st.append((~truth(st.pop()), "BOOL", no))
            pc += 1
        elif op == L.OP_ISNULL:
            st.append((st.pop()[2].copy(), "BOOL", no))
            pc += 1
        else:
            raise AssertionError(f"opcode {op}")
    assert len(st) == 1
    return truth(st[0])


def context(text, strings=None):
    a = C.parse(text)
    p = a.partitions[0]
    return L.make_context(a, p.queries[0], p, {} if strings is None else strings)


def random_columns(ctx, n, seed, with_nulls=True):
    """one random column per batch column of ctx (small value sets, so every compare hits both sides), and a null
    array for most columns"""
    rng = np.random.default_rng(seed)
    cols, nulls = [], []
    for c, (_, _, t) in enumerate(L.column_layout(ctx)):
        if t in ("INT", "LONG"):
            v = rng.integers(-3, 6, n)
        elif t in ("FLOAT", "DOUBLE"):
            v = rng.integers(-6, 12, n) / 2.0
        elif t == "STRING":
            v = rng.integers(0, 4, n)
        else:
            v = rng.integers(0, 2, n)
        cols.append(v.astype(NP[t]))
        nulls.append((rng.random(n) < 0.15).astype(np.uint8) if with_nulls and c % 4 != 2 else None)
    return cols, nulls


def host_masks(ctx, s, cols, nulls, n):
    d = ctx.app.streams[ctx.stream_ids[s]]
    cb = sum(len(ctx.app.streams[sid].attrs) for sid in ctx.stream_ids[:s])
    cd = {name: cols[cb + a] for a, (name, _) in enumerate(d.attrs)}
    nd = {name: nulls[cb + a] for a, (name, _) in enumerate(d.attrs) if nulls[cb + a] is not None}
    return [_range_mask(cond, d, cd, nd, ctx.strings, n) for cond, _ in ctx.key_ranges[s]]


ALL_TYPES = ("define stream S (s string, i int, l long, f float, d double, b bool, i2 int); "
             "partition with ({} of S) begin @info(name='q') from every e1=S -> e2=S[i>e1.i] "
             "select e1.i as a insert into M; end;")
CONDITIONS = [
    "i>1", "l<=2l", "f>=2.5f", "d<0.5", "s=='abc'", "s!='abc'", "b==true", "b",           # every attribute type
    "i>0 and f<3.0", "(i<0 or d>0.7)", "not (l>1l)", "not b", "b is null", "not (b is null)",
    "i!=2", "f!=1.5f", "i2==i",                                                                # != / == on a null
    "i>f", "i2<=f", "i<d", "i2==d",                                                            # INT with FLOAT / DOUBLE
    "s=='never sent'", "s!='never sent'",
    "l==f", "l!=f", "l>f",                                                                     # LONG with FLOAT
    "(i>0 and (f<3.0 or d>1.0)) and not (l==2l or b)",
]


def test_programs_equal_the_host_masks():
    strings = {"x0": 0, "abc": 1, "x2": 2, "x3": 3}
    ctx = context(ALL_TYPES.format(" or ".join(f"{c} as 'r{k}'" for k, c in enumerate(CONDITIONS))), strings)
    table = L.lower_ranges(ctx)
    assert [lab for _, lab, _ in table.ranges] == list(range(len(CONDITIONS)))   # written order, one code each
    n = 4000
    cols, nulls = random_columns(ctx, n, 5)
    want = host_masks(ctx, 0, cols, nulls, n)
    for k, (s, _, prog) in enumerate(table.ranges):
        assert s == 0
        got = interpret(prog, cols, nulls, n)
        assert np.array_equal(got, want[k]), CONDITIONS[k]
        if "never" not in CONDITIONS[k]:
            assert 0 < got.sum() < n, CONDITIONS[k]       # (the columns exercise both outcomes)
    never = CONDITIONS.index("s=='never sent'")
    assert not want[never].any() and want[never + 1].all()
    # no null array at all
    cols, nulls = random_columns(ctx, n, 6, with_nulls=False)
    want = host_masks(ctx, 0, cols, nulls, n)
    for k, (_, _, prog) in enumerate(table.ranges):
        assert np.array_equal(interpret(prog, cols, nulls, n), want[k]), CONDITIONS[k]


SHARED = ("define stream S (price float); define stream T (v float); "
          "partition with (price>=30 as 'hi' or price<30 as 'lo' of S, v<10 as 'small' or v>=30 as 'hi' or v<30 as 'lo' "
          "of T) begin @info(name='q') from every e1=S -> e2=T[v>e1.price] select e1.price as p, e2.v as v "
          "insert into M; end;")


def test_label_codes_are_shared_and_ranges_keep_written_order():
    table = L.lower_ranges(context(SHARED))
    assert table.labels == ["hi", "lo", "small"]
    assert [(s, table.labels[c]) for s, c, _ in table.ranges] == [(0, "hi"), (0, "lo"), (1, "small"), (1, "hi"),
                                                                  (1, "lo")]
    # programs read their own stream's batch column
    assert [p[3] for _, _, p in table.ranges] == [0, 0, 1, 1, 1]
    assert L.lower_ranges(context("define stream S (k int); partition with (k of S) begin @info(name='q') "
                                  "from every e1=S -> e2=S[k>e1.k] select e1.k as k insert into M; end;")) is None


def test_float_long_equality_compares_as_double():
    """v == 16777216.0f with v = 16777217 (LONG): (float) v rounds to 16777216.0f, so a float compare holds; the
    reference compares (double) v with (double) 16777216.0f (EqualCompareConditionExpressionExecutorLongFloat.java:
    36-38), 16777217.0 != 16777216.0: == does not hold and != holds."""
    text = ("define stream S (v long); partition with (v==16777216.0f as 'eq' or v!=16777216.0f as 'ne' or "
            "16777216.0f==v as 'qe' of S) begin @info(name='q') from every e1=S -> e2=S[v>e1.v] select e1.v as v "
            "insert into M; end;")
    ctx = context(text)
    cols = [np.array([16777217, 16777216, 16777215], np.int64)]
    want = [[False, True, False], [True, False, True], [False, True, False]]
    got = host_masks(ctx, 0, cols, [None], 3)
    assert [m.tolist() for m in got] == want
    table = L.lower_ranges(ctx)
    assert [interpret(p, cols, [None], 3).tolist() for _, _, p in table.ranges] == want
    assert [p[-1] for _, _, p in table.ranges] == [L.D_F64] * 3


# ------------------------------------------------------------------------------------------- CPU: ABI
def test_range_struct_layout_matches_c(tmp_path):
    from siddhi_amd import _native as N
    src = tmp_path / "sz.c"
    src.write_text('#include "siddhi_gpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(sg_range_desc), sizeof(sg_range_stats),'
                   ' offsetof(sg_range_desc, col_stream), offsetof(sg_range_desc, n_ranges),'
                   ' offsetof(sg_range_desc, range_label), offsetof(sg_range_desc, prog_len),'
                   ' offsetof(sg_range_desc, code_len), offsetof(sg_range_desc, code),'
                   ' offsetof(sg_range_stats, calls), offsetof(sg_range_stats, expand_ms), SG_MAX_RANGES);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, S = N.sg_range_desc, N.sg_range_stats
    assert got == [ct.sizeof(D), ct.sizeof(S), D.col_stream.offset, D.n_ranges.offset, D.range_label.offset,
                   D.prog_len.offset, D.code_len.offset, D.code.offset, S.calls.offset, S.expand_ms.offset,
                   N.SG_MAX_RANGES]


def test_library_exports_the_range_router():
    from siddhi_amd import _native as N
    lib = N.load_library()
    for s in ("sg_range_open", "sg_range_route", "sg_range_stats_get", "sg_range_close", "sg_range_last_error"):
        assert s in N.SYMBOLS and hasattr(lib, s), s


# ------------------------------------------------------------------------------------------- GPU: the router
class Harness:
    """One app on the host router (an oracle-engine runtime: _route_ranges is _range_route over _range_mask) and on a
    device router opened from lower_ranges of the same context."""

    def __init__(self, text):
        from siddhi_amd import _native as N
        self.N = N
        self.rt = SiddhiManager(engine=OracleEngine).createSiddhiAppRuntime(text)
        self.q = self.rt.queries[0]
        self.table = L.lower_ranges(self.q.ctx)
        self.router = N.RangeRouter(N.build_range_desc(self.table))
        self.hip = ct.CDLL("libamdhip64.so")
        self.widths = [np.dtype(NP[t]).itemsize for _, _, t in self.table.cols]

    def close(self):
        self.router.close()
        self.rt.shutdown()

    def _back(self, ptr, n, dtype):
        a = np.zeros(n, dtype)
        if n:
            assert ptr
            assert self.hip.hipMemcpy(ct.c_void_p(a.ctypes.data), ct.c_void_p(ptr), ct.c_size_t(a.nbytes), 2) == 0
        return a

    def device(self, b, keys, device_input=False, no_stream=False, no_key=False, no_index=False, no_nulls=False):
        """route b on the device with the key dictionary `keys` (label / key string -> id; updated like the host's):
        the routed batch copied back, as a Batch plus its key_bound.  no_stream / no_key / no_index pass that array of
        the sg_batch as NULL (every row stream 0 / key -1 / index base_index + row), no_nulls the array of null
        arrays itself (b must then have no null array)."""
        N = self.N
        labels = self.table.labels
        label_key = np.array([keys.get(lab, -1) for lab in labels], np.int32)
        first = len(keys)
        kb = int(b.key.max()) + 1 if b.n and b.key.max() >= 0 and not no_key else 0
        keep = []
        assert not no_nulls or all(x is None for x in b.nulls)
        stream, key = (None if no_stream else b.stream), (None if no_key else b.key)
        index = None if no_index else b.index
        if device_input:
            import torch
            dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
            ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
            idx = None if index is None else dev(index.view(np.int64))
            t = [dev(b.ts), dev(stream), dev(key), idx] + [dev(c) for c in b.cols] + [dev(x) for x in b.nulls]
            keep.append(t)
            torch.cuda.synchronize()
            nc = len(b.cols)
            sb = N.make_batch(b.n, b.base_index, ptr(t[0]), ptr(t[1]), ptr(t[2]), [ptr(x) for x in t[4:4 + nc]],
                              [ptr(x) for x in t[4 + nc:]], 1, kb, keep, index=ptr(t[3]))
        else:
            ptr = lambda a: 0 if a is None else a.ctypes.data   # noqa: E731
            sb = N.make_batch(b.n, b.base_index, ptr(b.ts), ptr(stream), ptr(key), [ptr(c) for c in b.cols],
                              [ptr(x) for x in b.nulls], 0, kb, keep, index=ptr(index))
        if no_nulls:
            sb.nulls = None
        out, after = self.router.route(sb, label_key, first)
        assert out.on_device == 1 and out.base_index == b.base_index
        new = {int(label_key[c]): lab for c, lab in enumerate(labels) if label_key[c] >= first}
        assert sorted(new) == list(range(first, after))
        for k in range(first, after):
            keys[new[k]] = k
        n = out.n
        P = ct.POINTER(ct.c_void_p)
        cp, npp = ct.cast(out.cols, P), ct.cast(out.nulls, P)
        cols = [self._back(cp[c], n, b.cols[c].dtype) for c in range(len(b.cols))]
        nulls = [None if b.nulls[c] is None else self._back(npp[c], n, np.uint8) for c in range(len(b.cols))]
        for c in range(len(b.cols)):
            assert b.nulls[c] is not None or not npp[c]        # NULL where the input's is
        r = Batch(n, out.base_index, self._back(out.ts, n, np.int64), self._back(out.stream, n, np.int32),
                  self._back(out.key, n, np.int32), cols, nulls, index=self._back(out.index, n, np.uint64))
        return r, out.key_bound

    def host(self, b, keys):
        self.rt.key_dicts[0] = keys
        return self.rt._route_ranges(0, self.q, b, b.stream)

    def check(self, b, keys=None, device_input=False):
        """device route == host route, field by field, and the same ids handed out; returns the device's batch"""
        keys = {} if keys is None else keys
        hk, dk = dict(keys), dict(keys)
        want = self.host(b, hk)
        got, key_bound = self.device(b, dk, device_input)
        assert list(dk.items()) == list(hk.items())          # the same labels took the same ids in the same order
        assert got.n == want.n
        for f in ("ts", "stream", "key", "index"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), f
        for c in range(len(b.cols)):
            assert got.cols[c].tobytes() == want.cols[c].tobytes(), f"column {c}"
            assert (got.nulls[c] is None) == (want.nulls[c] is None)
            if got.nulls[c] is not None:
                assert np.array_equal(got.nulls[c], want.nulls[c]), f"nulls {c}"
        kb_in = int(b.key.max()) + 1 if b.n and b.key.max() >= 0 else 0
        lab = [dk[x] for x in self.table.labels if x in dk]
        assert key_bound == max(kb_in, 1 + max(lab) if lab else 0)
        return got

    def check_reference(self, rows, b, keys=None, device_input=False, want=None, **null_arrays):
        """device route of b == range_ref.route of `rows` (the rows b was built from; `want` where the caller has
        routed them already), field by field, and the same dictionary in the same creation order; returns (the
        device's batch, the reference's routing)"""
        dk = {} if keys is None else dict(keys)
        given = None if b.index is None or null_arrays.get("no_index") else b.index
        if want is None:
            want = range_ref.route(self.rt.app, rows, keys=list(dk), base_index=b.base_index, indices=given,
                                   broadcast=False)
        got, key_bound = self.device(b, dk, device_input, **null_arrays)
        assert list(dk) == want.keys
        RC.assert_routed(got, want, b, self.rt.app, self.rt.strings)
        kb_in = int(b.key.max()) + 1 if b.n and b.key.max() >= 0 and not null_arrays.get("no_key") else 0
        lab = [dk[x] for x in self.table.labels if x in dk]
        assert key_bound == max(kb_in, 1 + max(lab) if lab else 0)
        return got, want


_harness = {}


def harness(text):
    if text not in _harness:
        _harness[text] = Harness(text)
    return _harness[text]


@pytest.fixture(scope="module", autouse=True)
def _close_harnesses():
    yield
    for h in _harness.values():
        h.close()
    _harness.clear()


# first 16 prices of every row-count case and, by hand, the ranges each holds (high: >=30, low: <30, tiny: <15)
P16 = [35.0, 20.0, 12.0, 31.0, 29.5, 14.5, 15.0, 30.0, 5.0, 45.0, 10.0, 22.0, 60.0, 1.0, 16.0, 33.0]
HOLDS3 = ["h", "l", "lt", "h", "l", "lt", "l", "h", "lt", "h", "lt", "l", "h", "lt", "l", "h"]
APPS = {1: app("price>=30 as 'hi'"), 3: app(RANGES),
        32: app(" or ".join(f"price>=0 as 'l{k}'" for k in range(32)))}


def hand_copies(R, n):
    """(row, key) of every copy of the first min(n, 16) rows, ids handed out from 0 in first-seen order"""
    rows = range(min(n, 16))
    if R == 1:       # 'hi' = 0
        return [(r, 0) for r in rows if "h" in HOLDS3[r]]
    if R == 32:      # every row holds l0..l31 in written order
        return [(r, k) for r in rows for k in range(32)]
    ids = {"h": 0, "l": 1, "t": 2}    # row 0 holds high, row 1 low, row 2 low then tiny
    return [(r, ids[x]) for r in rows for x in HOLDS3[r]]


def price_batch(n, seed=0, base=0):
    rng = np.random.default_rng(seed)
    price = np.round(rng.uniform(0, 60, n), 1).astype(np.float32)
    price[:min(n, 16)] = P16[:n]
    return Batch(n, base, np.arange(n, dtype=np.int64) * 3, np.zeros(n, np.int32), np.full(n, -1, np.int32),
                 [rng.integers(0, 3, n).astype(np.int32), price, np.arange(n, dtype=np.int32)], [None, None, None])


@pytest.mark.gpu
@pytest.mark.parametrize("R,n", [(3, 1), (3, 255), (3, 256), (3, 257), (3, 513), (3, (1 << 18) + 1),
                                 (1, 1), (1, 256), (1, 257), (1, 513), (32, 1), (32, 256), (32, 257), (32, 513)])
def test_router_equals_host_route_and_hand_rows(R, n):
    b = price_batch(n, seed=n + R, base=1000)
    got = harness(APPS[R]).check(b)
    hand = hand_copies(R, n)
    m = len(hand)
    assert int((got.index < 1000 + min(n, 16)).sum()) == m
    assert got.index[:m].tolist() == [1000 + r for r, _ in hand]
    assert got.key[:m].tolist() == [k for _, k in hand]
    assert got.cols[1][:m].tolist() == [P16[r] for r, _ in hand]
    assert got.cols[2][:m].tolist() == [r for r, _ in hand] and got.ts[:m].tolist() == [3 * r for r, _ in hand]
    assert set(got.stream.tolist()) <= {0}
    if R == 32 and n >= 256:
        assert got.n == 32 * n          # 8192 copies in every full tile


@pytest.mark.gpu
@pytest.mark.parametrize("playback", [False, True])
def test_router_batch_in_which_no_row_holds_a_range(playback):
    h = harness(app("price>=1000 as 'x' or price<-5 as 'y'", playback=playback))
    n = 300
    b = price_batch(n, seed=9)
    got = h.check(b)
    if playback:      # every row stays as one clock row
        assert got.n == n and got.stream.tolist() == [-1] * n and got.key.tolist() == [-1] * n
        assert got.index.tolist() == list(range(n)) and np.array_equal(got.cols[1], b.cols[1])
    else:
        assert got.n == 0


THREE = ("define stream S (price float, v long, w bool); define stream T (k int, d double); "
         "partition with (price>=30 as 'hi' or price<30 as 'lo' or v>5l as 'big' or w is null as 'now' of S, k of T) "
         "begin @info(name='q') from every e1=S -> e2=T[d>e1.price] select e1.price as p, e2.d as d "
         "insert into M; end;")


def three_stream_batch(n, seed):
    """rows of S (ranged), T (value keys 0..4) and stream -1 (clock rows), 4- and 8-byte columns, null arrays on
    some of them, and an explicit event index per row"""
    rng = np.random.default_rng(seed)
    stream = rng.choice(np.array([0, 0, 1, -1], np.int32), n)
    key = np.where(stream == 1, rng.integers(0, 5, n), -1).astype(np.int32)
    cols = [np.round(rng.uniform(0, 60, n), 1).astype(np.float32), rng.integers(0, 10, n).astype(np.int64),
            rng.integers(0, 2, n).astype(np.int32), rng.integers(0, 5, n).astype(np.int32), rng.uniform(0, 60, n)]
    nulls = [(rng.random(n) < 0.1).astype(np.uint8), None, (rng.random(n) < 0.2).astype(np.uint8), None,
             (rng.random(n) < 0.1).astype(np.uint8)]
    index = (np.uint64(5000) + np.cumsum(rng.integers(1, 4, n)).astype(np.uint64))
    return Batch(n, 77, np.cumsum(rng.integers(0, 5, n)).astype(np.int64), stream, key, cols, nulls, index=index)


@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
def test_router_three_streams_value_keys_and_given_index(device_input):
    h = harness(THREE)
    b = three_stream_batch(1500, 3)
    got = h.check(b, {f"{k}": k for k in range(5)}, device_input)     # T's value keys own ids 0..4
    # by hand, row by row: a T or clock row passes through; an S row has one copy per holding range, in written order
    ids = {"hi": None, "lo": None, "big": None, "now": None}
    nxt, want = 5, []
    for i in range(64):
        s = int(b.stream[i])
        if s != 0:
            want.append((int(b.index[i]), s, int(b.key[i])))
            continue
        p, v = (None if b.nulls[0][i] else float(b.cols[0][i])), int(b.cols[1][i])
        held = ([("hi")] if p is not None and p >= 30 else []) + (["lo"] if p is not None and p < 30 else []) + \
               (["big"] if v > 5 else []) + (["now"] if b.nulls[2][i] else [])
        for lab in held:
            if ids[lab] is None:
                ids[lab] = nxt
                nxt += 1
            want.append((int(b.index[i]), 0, ids[lab]))
    m = len(want)
    assert list(zip(got.index[:m].tolist(), got.stream[:m].tolist(), got.key[:m].tolist())) == want


@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
def test_router_host_and_device_input_agree(device_input):
    harness(APPS[3]).check(price_batch(513, seed=4), None, device_input)


FIRST_SEEN = ("{}define stream S (a int, b int); partition with (a>0 as 'x' or b>0 as 'y' of S) begin "
              "@info(name='q') from every e1=S -> e2=S[a>e1.a] select e1.a as a insert into M; end;")


@pytest.mark.gpu
def test_router_first_seen_ids_and_clock_rows():
    """the case of test_range_route_copies_ids_and_clock_rows: row 0 holds y; row 1 x, y; row 2 x; row 3 none; row 4
    x -- 'y' is seen first and takes 7, 'x' 8"""
    n = 5
    b = Batch(n, 100, np.arange(n, dtype=np.int64), np.zeros(n, np.int32), np.full(n, -1, np.int32),
              [np.array([0, 1, 1, 0, 1], np.int32), np.array([1, 1, 0, 0, 0], np.int32)], [None, None])
    seven = {f"k{k}": k for k in range(7)}
    for playback in (False, True):
        h = harness(FIRST_SEEN.format("@app:playback " if playback else ""))
        keys = dict(seven)
        got, key_bound = h.device(b, keys)
        assert keys["y"] == 7 and keys["x"] == 8 and len(keys) == 9 and key_bound == 9
        if playback:
            assert got.index.tolist() == [100, 101, 101, 102, 103, 104]
            assert got.stream.tolist() == [0, 0, 0, 0, -1, 0] and got.key.tolist() == [7, 8, 7, 8, -1, 8]
        else:
            assert got.index.tolist() == [100, 101, 101, 102, 104]
            assert got.key.tolist() == [7, 8, 7, 8, 8]
        h.check(b, dict(seven))


@pytest.mark.gpu
def test_router_known_label_keeps_its_key_and_new_ones_start_at_next_key():
    h = harness(APPS[3])
    keys = {f"k{k}": k for k in range(6)}
    keys["low"] = 6                     # next_key = 7
    b = price_batch(400, seed=2)
    got = h.check(b, keys)
    # rows 0..2 are 35 (high), 20 (low), 12 (low, tiny): high takes 7, tiny 8, low stays 6
    assert got.key[:4].tolist() == [7, 6, 6, 8]


@pytest.mark.gpu
def test_router_reuses_and_regrows_its_buffers():
    h = harness(APPS[3])
    keys = {}
    for n, seed in ((300, 1), (70000, 2), (100, 3)):
        b = price_batch(n, seed=seed, base=10 * n)
        h.check(b, keys)
        h.host(b, keys)          # (check leaves `keys` as it was: carry the ids into the next call)
    st = h.router.stats()
    assert st.calls >= 3 and st.rows >= 70400 and st.copies > st.rows and st.hold_ms > 0 and st.expand_ms > 0


def test_router_refuses_a_bad_descriptor():
    """sg_range_open checks the descriptor before it touches the device, so this runs without one"""
    from siddhi_amd import _native as N
    table = L.lower_ranges(context(app()))
    for field, value, code in (("n_ranges", 0, -1), ("n_ranges", 33, -1), ("n_labels", 0, -1), ("abi_version", 3, -1),
                               ("code_len", 2, -1)):
        d = N.build_range_desc(table)
        setattr(d, field, value)
        with pytest.raises(N.SgError) as e:
            N.RangeRouter(d)
        assert e.value.code == code
    d = N.build_range_desc(table)
    d.code[3] = 9                       # a column the batch does not have
    with pytest.raises(N.SgError):
        N.RangeRouter(d)
    # a program deeper than the VM stack: 17 operands before the first operator
    deep = [L.OP_CONST, L.TYPE_CODE["INT"], 1] * 17 + [L.OP_CMP, 0, L.D_I64] + [L.OP_AND] * 15
    table.ranges[0] = (0, 0, deep)
    with pytest.raises(N.SgError) as e:
        N.RangeRouter(N.build_range_desc(table))
    assert e.value.code == N.SG_EUNSUPPORTED


# ------------------------------------------------------------------------------------------- GPU: against range_ref
# Expected values below come from range_ref.route, the row-at-a-time restatement that shares no code with either router.
@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
@pytest.mark.parametrize("k", range(len(RC.TYPED_APPS)))
def test_router_types_and_domains_equal_reference(k, device_input):
    """the all-type apps of test_range_reference.py (column pairs x operators, edge constants, STRING / BOOL, `is null`,
    nested forms; edge-value pools with nulls) on the device"""
    case = RC.typed_case(k)
    h = harness(case.text)
    b = RC.batch_of(h.rt.app, case.rows, h.rt.strings, base=500)
    h.check_reference(case.rows, b, None, device_input, want=case.want)


def prog_depth(prog):
    """operand stack depth of a postfix range program (what sg_range_open sizes the hold kernel's stack from)"""
    sp = mx = pc = 0
    while pc < len(prog):
        op = prog[pc]
        push, words = {L.OP_VAR: (1, 5), L.OP_CONST: (1, 3), L.OP_CMP: (-1, 3), L.OP_AND: (-1, 1), L.OP_OR: (-1, 1),
                       L.OP_NOT: (0, 1), L.OP_ISNULL: (0, 1)}[op]
        sp, pc = sp + push, pc + words
        mx = max(mx, sp)
    return mx


# atoms of every operand type (depth <= 2 each); the innermost one compares a LONG with a FLOAT column, both with nulls,
# so at the deepest point the stack holds truth values, an i64 and an f64 operand and null flags at once
ATOMS = ["i>0", "f<3.0", "l is null", "d>=0.5", "b", "s!='abc'", "i2!=2", "not (f2 is null)", "l>f", "d2<2.0", "i==f",
         "l2!=9007199254740993l", "f2>=d", "i<=l"]
INNERMOST = "l2<=f2"


def nested(m):
    """(c1 and (c2 or (c3 and ... cm))), right-nested: every level keeps one more truth value on the stack, so m
    atoms need depth m + 1"""
    atoms = ATOMS[:m - 1] + [INNERMOST]
    e = atoms[-1]
    for j in range(m - 2, -1, -1):
        e = f"({atoms[j]} {'and' if j % 2 == 0 else 'or'} {e})"
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
@pytest.mark.parametrize("depth", [2, 4, 8, 16])
def test_router_every_hold_kernel_depth(depth, device_input):
    """launch_hold picks k_rr_hold<2 | 4 | 8 | 16> from the deepest program: one app per instantiation"""
    text = RC.TYPED.format(f"{nested(depth - 1)} as 'deep' or i>0 as 'pos' or l is null as 'nul'")
    h = harness(text)
    assert max(prog_depth(p) for _, _, p in h.table.ranges) == depth
    assert sum(len(p) for _, _, p in h.table.ranges) <= L.MAX_CODE
    rows = RC.typed_rows(1000, 40 + depth)
    b = RC.batch_of(h.rt.app, rows, h.rt.strings, base=7)
    _, want = h.check_reference(rows, b, None, device_input)
    deep = sum(1 for r in want.rows if want.keys[r[2]] == "deep")
    assert 0 < deep < len(rows)


FIRST = ("define stream S (a int, b int, c int, r int); partition with ({} of S) begin @info(name='q') "
         "from every e1=S -> e2=S[a>e1.a] select e1.a as a insert into M; end;")
FIRST_LABELS = {2: FIRST.format("a>0 as 'A' or b>0 as 'B'"), 3: FIRST.format("a>0 as 'A' or b>0 as 'B' or c>0 as 'C'")}


def first_rows(n, firsts):
    """rows of S whose column j is 0 before row firsts[j] and 1 in that row: label j is first held in row firsts[j].
    After it the label that comes q-th in first-held order holds every row with row % 8 == 6 - 2 q, so in every later
    wave and tile the labels' first holders come in the REVERSE order: a router that read a label's first holder from
    a later wave or tile than the first would hand out other ids.  Column r is the row number."""
    order = sorted(range(len(firsts)), key=lambda j: (firsts[j], j))
    return [(0, 2 * r, [int(r == f or (r > f and r % 8 == 6 - 2 * order.index(j))) for j, f in enumerate(firsts)] +
             [0] * (3 - len(firsts)) + [r]) for r in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("firsts", [(63, 64), (64, 63), (255, 256), (256, 255), (191, 192), (300, 300), (599, 0),
                                    (512, 511), (256, 255, 64), (300, 300, 300), (599, 0, 320), (130, 447, 129)])
def test_router_first_holders_away_from_row_zero(firsts):
    """three tiles of 256 rows; the first holders sit in other waves than wave 0 and other tiles than tile 0, on both
    sides of a wave and a tile border: the per-wave table, the lowest-wave loop and the minimum across tiles decide the
    ids.  A row that holds two new labels gives them ids in written order."""
    h = harness(FIRST_LABELS[len(firsts)])
    rows = first_rows(600, firsts)
    b = RC.batch_of(h.rt.app, rows, h.rt.strings, base=100)
    got, want = h.check_reference(rows, b)
    order = sorted(range(len(firsts)), key=lambda j: (firsts[j], j))       # by hand: first row, then written order
    assert want.keys == ["ABC"[j] for j in order]
    for j, f in enumerate(firsts):
        copies = got.key == order.index(j)
        assert int(got.index[copies].min()) == 100 + f and copies.sum() >= 1 + (599 - f) // 8


@pytest.mark.gpu
def test_router_first_holder_with_one_label_known():
    """'A' is in the dictionary (label_key >= 0: the hold kernel skips it), 'B' is new and first held in tile 1"""
    h = harness(FIRST_LABELS[2])
    rows = first_rows(600, (130, 447))
    b = RC.batch_of(h.rt.app, rows, h.rt.strings, base=0)
    got, want = h.check_reference(rows, b, {"k0": 0, "A": 1, "k2": 2})
    assert want.keys == ["k0", "A", "k2", "B"] and set(got.key.tolist()) == {1, 3}


@pytest.mark.gpu
def test_router_32_labels_first_held_in_reverse_written_order():
    """label k is first held in row 560 - 17 k: the ids come out in row order, the reverse of the written order"""
    h = harness(FIRST.format(" or ".join(f"r>={560 - 17 * k} as 'l{k}'" for k in range(32))))
    rows = first_rows(600, ())
    b = RC.batch_of(h.rt.app, rows, h.rt.strings, base=0)
    got, want = h.check_reference(rows, b)
    assert want.keys == [f"l{k}" for k in range(31, -1, -1)]
    assert got.n == sum(600 - (560 - 17 * k) for k in range(32))


def shared_rows(n=600):
    """S (even rows) holds 'lo' from row 0 and 'hi' from row 400 on; T (odd rows) holds 'lo', 'hi' from row 71 on and
    'small' from row 301 on: 'hi' is first held through T's range, written after S's, in an earlier row"""
    rng = np.random.default_rng(2)
    rows = []
    for r in range(n):
        u = rng.random()
        if r % 2 == 0:
            rows.append((0, r, [50.0 if r >= 400 and (r == 400 or u < 0.5) else 20.0]))
        elif r >= 301 and (r == 301 or u < 0.3):
            rows.append((1, r, [5.0]))
        else:
            rows.append((1, r, [40.0 if r >= 71 and (r == 71 or u < 0.65) else 15.0]))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
def test_router_label_shared_by_two_streams_first_held_through_the_later_one(device_input):
    h = harness(SHARED)
    rows = shared_rows()
    b = RC.batch_of(h.rt.app, rows, h.rt.strings, base=0)
    got, want = h.check_reference(rows, b, None, device_input)
    assert want.keys == ["lo", "hi", "small"]            # rows 0, 71 and 301
    hi = got.key == 1
    assert int(got.index[hi].min()) == 71 and set(got.stream[hi].tolist()) == {0, 1}


UNRANGED = ("define stream S (a int, b int); define stream U (u int); partition with (a>0 as 'A' or b>0 as 'B' of S) "
            "begin @info(name='q') from every e1=S -> e2=U[u>e1.a] select e1.a as a insert into M; end;")


@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
@pytest.mark.parametrize("absent", ["stream", "key", "index", "nulls", "none"])
def test_router_optional_arrays(absent, device_input):
    """sg_batch.stream / key / index and the array of null arrays may each be NULL"""
    rng = np.random.default_rng(5)
    n = 700
    if absent == "key":          # rows of U pass through with key -1
        h = harness(UNRANGED)
        rows = [(0, r, [int(rng.integers(0, 2)), int(rng.integers(-1, 2))]) if rng.random() < 0.6 else (1, r, [r])
                for r in range(n)]
    elif absent == "nulls":
        h = harness(RC.TYPED.format(f"{nested(3)} as 'deep' or i>0 as 'pos' or f2>=d as 'fd'"))
        rows = RC.typed_rows(n, 9, null_rate=0.0)
    else:
        h = harness(FIRST_LABELS[2])
        rows = first_rows(n, (130, 70))
    index = None
    if absent in ("index", "none"):      # given here, and left out below for "index"
        index = np.uint64(9000) + np.cumsum(rng.integers(1, 4, n)).astype(np.uint64)
    b = RC.batch_of(h.rt.app, rows, h.rt.strings, base=50, index=index)
    got, want = h.check_reference(rows, b, None, device_input, **({} if absent == "none" else {f"no_{absent}": True}))
    assert got.n > n // 8
    if absent == "key":
        assert set(got.key[got.stream == 1].tolist()) == {-1} and (got.stream == 1).sum() == sum(s for s, _, _ in rows)
    if absent == "index":
        assert got.index.max() < 50 + n
    if absent == "none":
        assert got.index.min() > 9000


# ------------------------------------------------------------------------------------------- GPU: end to end
def run_columns(engine, text, sends, device_ranges=True, snapshot_after=None):
    """send_columns every (stream, cols) of `sends`; returns (delivered rows, rows the engine was pushed, the range
    router's stats or None).  snapshot_after = k: after k sends the state moves into a fresh runtime."""
    pushed, got, stats = [0], [], []

    def make():
        rt = SiddhiManager(engine=engine).createSiddhiAppRuntime(text)
        rt.device_ranges = device_ranges

        class CB(QueryCallback):
            def receive(self, ts, ins, rem):
                got.extend((ts, tuple(e.data)) for e in ins)

        rt.addCallback("q", CB())
        rt.start()
        eng = rt.queries[0].engine
        inner = eng.push

        def counting_push(b):
            pushed[0] += b.n
            inner(b)
        eng.push = counting_push
        return rt

    rt = make()

    def collect(rt):
        r = getattr(rt.queries[0].engine, "range_router", None)
        if r is not None:
            stats.append(r.stats())

    for k, (stream, cols) in enumerate(sends):
        if snapshot_after == k:
            blob = rt.snapshot()
            collect(rt)
            rt.shutdown()
            rt = make()
            rt.restore(blob)
        rt.getInputHandler(stream).send_columns(**cols)
    collect(rt)
    rt.shutdown()
    return got, pushed[0], stats


def price_columns(rows):
    return dict(ts=np.array([t for t, _ in rows]), symbol=np.array([r[0] for _, r in rows]),
                price=np.array([r[1] for _, r in rows], np.float32), volume=np.array([r[2] for _, r in rows], np.int32))


def e2e(text, sends, min_rows, snapshot_after=None):
    from siddhi_amd._native import GpuEngine
    want, routed, _ = run_columns(OracleEngine, text, sends)
    assert len(want) >= min_rows
    got, pushed, stats = run_columns(GpuEngine, text, sends, snapshot_after=snapshot_after)
    assert got == want
    assert pushed == 0                               # every batch went through push_ranges
    assert sum(s.calls for s in stats) == len(sends) and sum(s.copies for s in stats) == routed
    got, pushed, stats = run_columns(GpuEngine, text, sends, device_ranges=False, snapshot_after=snapshot_after)
    assert got == want
    assert pushed == routed and sum(s.calls for s in stats) == 0


@pytest.mark.gpu
def test_e2e_three_ranges_column_path():
    rows = [r for r in _random_rows(20000, 3) if r[1][1] is not None]
    e2e(app(within="within 1 sec"), [("S", price_columns(rows))], 1000)


@pytest.mark.gpu
def test_e2e_playback_absence_with_clock_rows():
    rng = np.random.default_rng(11)
    n = 20000
    cols = dict(ts=np.cumsum(rng.integers(0, 300, n)), id=rng.integers(0, 50, n).astype(np.int64),
                price=rng.choice(np.array([5.0, 30.0, 70.0], np.float32), n))
    e2e(ABSENT_APP, [("S", cols)], 500)


@pytest.mark.gpu
def test_e2e_two_streams_sharing_a_label():
    rng = np.random.default_rng(12)
    n, chunk = 20000, 1000
    ts = np.cumsum(rng.integers(0, 20, n))
    val = np.round(rng.uniform(0, 60, n), 1).astype(np.float32)
    sends = []
    for lo in range(0, n, chunk):     # S and T take turns, so no instance collects thousands of waiting partials
        name, attr = (("S", "price"), ("T", "v"))[(lo // chunk) % 2]
        sends.append((name, {"ts": ts[lo:lo + chunk], attr: val[lo:lo + chunk]}))
    e2e(SHARED, sends, 1000)


@pytest.mark.gpu
def test_e2e_second_call_introduces_a_label_and_snapshot_between_calls():
    rows = [r for r in _random_rows(6000, 21) if r[1][1] is not None]
    first = [r for r in rows[:3000] if r[1][1] >= 30]           # only 'high' is held
    sends = [("S", price_columns(first)), ("S", price_columns(rows[3000:]))]
    text = app(within="within 1 sec")
    e2e(text, sends, 200)
    e2e(text, sends, 200, snapshot_after=1)


@pytest.mark.gpu
def test_e2e_is_null_of_a_float_attribute_column_path():
    """`is null` of a FLOAT attribute in a range condition (refused before the fix in lowering._check_range_cond), alone
    and under not / and, through send_columns on the device route and the host route.  send_columns carries no nulls,
    so no row holds 'missing' and `not (price is null)` holds on every row: this shows that the app is accepted and
    that ISNULL is false on the device for a column without a null array.  Rows that hold 'missing' are routed on the
    device in the typed apps above and run end to end in the row-path test below."""
    rows = [r for r in _random_rows(2000, 5) if r[1][1] is not None]
    ranges = "price is null as 'missing' or not (price is null) and price>=30 as 'hi' or price<30 as 'lo'"
    e2e(app(ranges, within="within 1 sec"), [("S", price_columns(rows))], 100)


IS_NULL_ROWS_APP = ("define stream S (symbol string, price float, volume int); "
                    "partition with (price is null as 'missing' or not (price is null) and price>=30 as 'hi' or "
                    "price<30 as 'lo' of S) begin @info(name='q') from every e1=S -> e2=S[volume>e1.volume] "
                    "select e1.volume as v1, e2.volume as v2, e2.price as p2 insert into M; end;")


@pytest.mark.gpu
def test_e2e_is_null_of_a_float_attribute_row_path_with_null_prices():
    """the same ranges on the row path, which carries nulls: about 30 % of the rows have no price and hold 'missing'.
    The MI355X engine is pushed the reference router's copies, 'missing' gets its id in the reference's place, and it
    delivers what the oracle engine delivers, matches inside 'missing' (p2 null) among them."""
    from siddhi_amd._native import GpuEngine
    rows = RC.price_rows(2000, 5)
    assert 400 < sum(v[1] is None for _, _, v in rows) < 800
    assert "missing" in range_ref.route(C.parse(IS_NULL_ROWS_APP), rows).keys
    want = RC.check_flush_granularity(OracleEngine, IS_NULL_ROWS_APP, rows, 100, plans={"one flush": set()})
    assert sum(d[2] is None for _, d in want) >= 20 and sum(d[2] is not None for _, d in want) >= 20
    RC.check_flush_granularity(GpuEngine, IS_NULL_ROWS_APP, rows, delivered=want,
                               plans=RC.flush_plans(len(rows), every_row=False, pieces=40))


@pytest.mark.gpu
def test_e2e_mixed_flush_row_path():
    """value keys, range labels and an unpartitioned stream in one partition on the row path: however the rows are
    flushed, the MI355X engine is pushed the reference router's copies and delivers what the oracle engine delivers
    when every row is flushed on its own"""
    from siddhi_amd._native import GpuEngine
    three = [(1, 0, [1]), (2, 1, [7]), (0, 2, [5])]
    assert RC.check_flush_granularity(GpuEngine, RC.MIXED3, three) == []
    rows = RC.mixed_rows(2000, 8, rate=0.01)
    want = RC.check_flush_granularity(OracleEngine, RC.MIXED, rows, 200, plans={"every row": set(range(len(rows)))})
    RC.check_flush_granularity(GpuEngine, RC.MIXED, rows, plans=RC.flush_plans(len(rows), every_row=False, pieces=40),
                               delivered=want)
