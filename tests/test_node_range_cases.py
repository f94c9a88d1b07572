"""CPU guards of the cases test_node_ranges.py runs on the GPU (node_range_cases.py), and of the two entry points.

A GPU case is only worth its seconds if its expectation is not empty, if the events it says hold two ranges do, and if
the labels it says live on different shards do under mix64.  Its expectation comes from range_ref.route with the oracle
engine; here the product's host router (runtime._route_ranges inside an oracle-engine runtime) must arrive at the same
copies, the same dictionary and the same delivered rows."""
import os
import struct
import subprocess

import pytest

import node_range_cases as NC
import range_cases as RC
from oracle import OracleEngine
from siddhi_amd import lowering as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(NC.CASES)


def decoded(p: NC.Prepared):
    """the oracle's outputs as the runtime delivers them: (timestamp, data tuple) per match"""
    types = [t for (_, _, _, t) in p.nfa.select]
    back = {i: s for s, i in p.strings.items()}
    rows = []
    for r in range(len(p.want)):
        data = []
        for k, t in enumerate(types):
            v = int(p.want.vals[r, k])
            if p.want.vnull[r, k]:
                v = None
            elif t == "FLOAT":
                v = struct.unpack("<f", struct.pack("<I", v & 0xffffffff))[0]
            elif t == "DOUBLE":
                v = struct.unpack("<d", struct.pack("<q", v))[0]
            elif t == "STRING":
                v = back[v]
            elif t == "BOOL":
                v = bool(v)
            data.append(v)
        rows.append((int(p.want.ts[r]), tuple(data)))
    return rows


@pytest.mark.parametrize("name", NAMES)
def test_case_is_worth_running(name):
    p = NC.prepared(name)
    c = p.case
    assert len(p.want) > 0
    for lo, hi in NC.pieces(p):          # every push delivers something, the pushes of one row included
        assert ((p.want.trigger >= c.base + lo) & (p.want.trigger < c.base + hi)).any(), (lo, hi)
    assert set(p.table.labels) <= set(c.raw)
    held = p.held()
    assert sum(len(h) for h in held) == sum(1 for r in p.routed.rows if r[2] >= 0)
    for a, b in c.apart:
        for g in (2, 3, 4):
            assert NC.shard(c.raw[a], g) != NC.shard(c.raw[b], g), (a, b, g)
        if c.together:
            both = [(i, h) for i, h in enumerate(held) if a in h and b in h]
            assert both, (a, b)
            for i, h in both:                    # the copies of one event come in the written order of its stream's ranges
                order = [p.table.labels[lab] for s, lab, _ in p.table.ranges if s == c.rows[i][0]]
                pos = [order.index(lab) for lab in h]
                assert pos == sorted(pos)
    if c.together:
        assert any(len(h) >= 2 for h in held)
    # the triggers are event indices of the pushed rows, several matches of one event included
    assert p.want.trigger.min() >= c.base and p.want.trigger.max() < c.base + len(c.rows)


def test_what_the_special_cases_claim():
    p = NC.prepared("core")
    first = [h for h in p.held()[:500]]
    assert not any("tiny" in h for h in first) and any("tiny" in h for h in p.held()[500:])
    assert p.nfa.shape == L.SHAPE_EVERY_NEXT_CMP and not p.nfa.out_progs      # the closed form the host fill serves
    o = NC.prepared("order")
    assert o.routed.keys == ["low", "tiny"]                                   # first seen: low, then tiny
    assert [o.table.labels[c] for _, c, _ in o.table.ranges] == ["tiny", "low"]   # written: tiny, then low
    t = o.want.trigger
    k = o.want.key
    same = [(int(k[i]), int(k[i + 1])) for i in range(len(t) - 1) if t[i] == t[i + 1]]
    assert (1, 0) in same and (0, 1) not in same      # one event's matches: tiny's (key 1) before low's (key 0)
    a = NC.prepared("all32")
    assert len(a.routed.rows) == 32 * 2049 and all(len(h) == 32 for h in a.held())
    assert all(len(h) == 1 for h in NC.prepared("one_of_32").held())
    ch = NC.prepared("chunks")
    assert all(h == [] for h in ch.held()[1000:1060])                         # chunks of 5 rows with no copy at all
    assert len({NC.shard(r, 4) for r in ch.case.raw.values()}) < 4            # a shard that never gets a row
    v = NC.prepared("value_and_ranges")
    assert v.case.raw["7"] == v.label_raw[v.table.labels.index("7")]
    seven = v.routed.keys.index("7")
    assert {r[1] for r in v.routed.rows if r[2] == seven} == {0, 1}           # one instance, rows of both streams
    u = NC.prepared("unread_column")
    assert 0 not in [c for c, _ in _ret_cols(u)]                              # column 0 = symbol: conditions only
    n = NC.prepared("null_condition")
    nulls = [i for i, (_, _, v) in enumerate(n.case.rows) if v[1] is None]
    assert nulls and all(n.held()[i] == ["ne"] for i in nulls)


def _ret_cols(p):
    """(batch column, type) of every attribute the query retains"""
    from siddhi_amd import _native as N
    d = N.build_desc(p.nfa)
    return [(d.ret_col[k], d.ret_type[k]) for k in range(d.n_ret)]


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("slice")] + ["slice2049x2"])
def test_host_router_agrees_with_the_reference(name):
    p = NC.prepared(name)
    c = p.case
    got, keys, pushed = RC.run_flushed(OracleEngine, c.text, c.rows, set(x - 1 for x in c.cuts))
    assert keys == p.routed.keys
    assert pushed == [(r[0] - c.base,) + r[1:4] for r in p.routed.rows]
    assert got == decoded(p)


# ------------------------------------------------------------------------------------------- the entry points
def test_library_exports_the_node_range_calls(tmp_path):
    from siddhi_amd import _native as N
    lib = N.load_library()
    for s in ("sg_node_set_ranges", "sg_node_range_stats_get"):
        assert s in N.SYMBOLS and hasattr(lib, s), s
    assert hasattr(N.Node, "set_ranges") and hasattr(N.Node, "range_stats")
    src = tmp_path / "nr.c"
    src.write_text('#include "siddhi_gpu.h"\n#include <stdio.h>\nint main(){'
                   'int (*a)(sg_node*, const sg_range_desc*, const int64_t*) = sg_node_set_ranges;'
                   'int (*b)(const sg_node*, sg_range_stats*) = sg_node_range_stats_get;'
                   'sg_range_stats st; printf("%d %d %d\\n", a(NULL, NULL, NULL), b(NULL, &st), SG_ABI_VERSION);'
                   'return 0;}')
    exe = tmp_path / "nr"
    libdir = os.path.dirname(N.LIB_PATH)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
                    "-l:" + os.path.basename(N.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["-1", "-1", "4"]      # SG_EINVAL for the null node, twice; the ABI version did not move
