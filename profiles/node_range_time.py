"""Time N rows of the three-range app through sg_node_push: ranges routed inside the node against copies expanded
on the host beforehand.

    python profiles/node_range_time.py [--rows 20000000] [--reps 5] [--gpus 1,2] [--only new] [--out FILE.json]

(a) new: the raw rows, in pinned host memory, go to a node with sg_node_set_ranges; the GPUs hold, count and scatter the
    copies.
(b) old: what a caller had to do before: every row expanded into its copies on the host (the product's host router,
    runtime._range_mask / _range_route; its time is reported separately, once), the copies copied into pinned memory and
    pushed as ordinary rows of a value partition, raw_key = the label's raw key, one event index per copy.
Both deliver the same matches ((b)'s triggers are copy ordinals; mapped back through the copies' event indices they
must equal (a)'s).  Per G the two alternate in one process after one warm-up each; reported are the medians and the
spread (min, max) of sg_node_stats.total_ms, the H2D bytes, and the node's range stats.  G > 1 runs G shards on device
0: the shards share one device, so it shows the cost of the exchange's extra passes, not a speed-up.
Timestamps are 2 s apart (the pattern's `within` is 1 s) except one pair in a thousand, so matching and delivery stay a
small part of the push.  Under `rocprofv3 --kernel-trace --stats` with --only new --reps 1 the trace holds the per-chunk
times of k_rr_hold, k_xrcount and k_xrscatter (profiles/kstats.py sums them).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from siddhi_amd import _native as N  # noqa: E402
from siddhi_amd import compiler as C  # noqa: E402
from siddhi_amd import lowering as L  # noqa: E402
from siddhi_amd.runtime import Batch, _range_mask, _range_route  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "profiles"))
from range_route_time import APP, columns  # noqa: E402

LABEL_RAW = {"high": 1000, "low": 1001, "tiny": 1002}   # (low and tiny on different shards at G = 2, 3, 4)


def pinned(a):
    p = N.PinnedArray(len(a), a.dtype)
    p.array[:] = a
    return p


def node_batch(n, ts, raw, cols, keep):
    keep += [ts, raw] + cols
    return N.make_node_batch(n, 0, ts.array.ctypes.data, 0, raw.array.ctypes.data, [c.array.ctypes.data for c in cols],
                             [0] * len(cols), keep)


def one_push(desc, gpus, batch, n, sink, ranges=None):
    node = N.Node(desc, n_gpus=gpus, devices=[0] * gpus, threads=16)
    if ranges is not None:
        node.set_ranges(*ranges)
    t0 = time.perf_counter()
    got = node.push(batch, sink.struct, sink.cap)
    wall = (time.perf_counter() - t0) * 1e3
    st = node.stats()
    res = {"wall_ms": wall, "total_ms": st["total_ms"], "reserve_ms": st["reserve_ms"], "h2d_bytes": st["h2d_bytes"],
           "d2h_bytes": st["d2h_bytes"], "chunks": st["chunks"], "matches": got,
           "shard_rows": st["shard_rows"][:gpus]}
    if ranges is not None:
        rs = node.range_stats()
        res.update(range_rows=rs.rows, range_copies=rs.copies)
    node.close()
    return res, sink.trigger[:got].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpus", default="1,2")
    ap.add_argument("--only", choices=["new", "both"], default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.rows
    app = C.parse(APP)
    part = app.partitions[0]
    ctx = L.make_context(app, part.queries[0], part, {})
    nfa = L.lower(ctx)
    desc = N.build_desc(nfa)
    table = L.lower_ranges(ctx)
    ranges = (N.build_range_desc(table), np.array([LABEL_RAW[x] for x in table.labels], np.int64))
    cols = columns(n)
    keep = []
    host_cols = [cols["symbol"], cols["price"], cols["volume"]]
    new_batch = node_batch(n, pinned(cols["ts"]), pinned(np.zeros(n, np.int64)), [pinned(c) for c in host_cols], keep)
    out = {"rows": n, "reps": a.reps}
    old_batch, index = None, None
    if a.only == "both":
        # (b)'s copies: the host router, timed once (it is the same work every time)
        t0 = time.perf_counter()
        d = app.streams["S"]
        names = [x for x, _ in d.attrs]
        masks = np.stack([_range_mask(cond, d, dict(zip(names, host_cols)), {}, {}, n) for cond, _ in ctx.key_ranges[0]])
        labels = [lab for _, lab in ctx.key_ranges[0]]
        ids = {}
        b = Batch(n, 0, cols["ts"], np.zeros(n, np.int32), np.full(n, -1, np.int32), host_cols, [None] * 3)
        rb = _range_route(b, b.stream, {0: (labels, masks)}, lambda lab: ids.setdefault(lab, len(ids)))
        raw_of_id = np.zeros(len(ids), np.int64)
        for lab, i in ids.items():
            raw_of_id[i] = LABEL_RAW[lab]
        raw = raw_of_id[rb.key]
        out["host_expand_ms"] = (time.perf_counter() - t0) * 1e3
        index = rb.index if rb.index is not None else np.arange(rb.n, dtype=np.uint64)
        old_batch = node_batch(rb.n, pinned(rb.ts), pinned(raw), [pinned(c) for c in rb.cols], keep)
        out["copies"] = int(rb.n)
        print("host expansion", round(out["host_expand_ms"], 1), "ms,", rb.n, "copies", flush=True)
    sink = N.ColumnSink(nfa, n // 50 + 1024, pinned=True, fields=("trigger", "ts", "key", "group"))
    for g in [int(x) for x in a.gpus.split(",")]:
        runs = {"new": [], "old": []}
        want = None
        for rep in range(a.reps + 1):            # rep 0 warms both up
            for which in (("old", "new") if a.only == "both" else ("new",)):
                if which == "new":
                    res, trig = one_push(desc, g, new_batch, n, sink, ranges)
                else:
                    res, trig = one_push(desc, g, old_batch, out["copies"], sink)
                    trig = index[trig.astype(np.int64)]
                if want is None:
                    want = trig
                assert np.array_equal(trig, want), "the two routes delivered different matches"
                if rep:
                    runs[which].append(res)
                print(f"G={g}", which, "warm-up" if not rep else f"rep {rep}",
                      {k: (round(v, 2) if isinstance(v, float) else v) for k, v in res.items()}, flush=True)
        summary = {}
        for which, rs in runs.items():
            if not rs:
                continue
            t = [r["total_ms"] for r in rs]
            summary[which] = {"total_ms_median": statistics.median(t), "total_ms_min": min(t), "total_ms_max": max(t),
                              "wall_ms_median": statistics.median(r["wall_ms"] for r in rs),
                              "h2d_bytes": rs[0]["h2d_bytes"], "d2h_bytes": rs[0]["d2h_bytes"], "chunks": rs[0]["chunks"],
                              "matches": rs[0]["matches"], "shard_rows": rs[0]["shard_rows"]}
            if which == "new":
                summary[which].update(range_rows=rs[0]["range_rows"], range_copies=rs[0]["range_copies"])
        out[f"G{g}" + (" (shards share one device)" if g > 1 else "")] = summary
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
