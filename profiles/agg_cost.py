"""Time the selector's aggregation stage on a config's stream held in HBM.

    python profiles/agg_cost.py --mode agg|base --config C2|C5 [--events N] [--steps 3] [--root TREE] [--out FILE.json]
    python profiles/agg_cost.py --mode serial --events N          # sum(double), unpartitioned, no group by

--mode agg   the aggregate query (the issue's app on the config's stream, `having` removed; StockStream has no volume
             column, so sum() takes e2.id):  select e1.symbol as s, count() as n, sum(e2.id) as vol,
             avg(e2.price - e1.price) as gain, max(e2.price) as hi group by e1.symbol
--mode base  the base app: the same pattern with the aggregators' arguments as plain select columns.  Run it with
             --root pointing at a checkout of the parent commit (built) for the baseline.
--mode serial  C1's stream (one key) through `select sum(e2.price + 0.0) as s`: one group in all, so k_agg_serial walks
             the push's matches on one lane -- the documented worst case.

Every step resets the handle and pushes the whole batch once (on_device); reported: the median wall time of a push
(stream synchronised), the HIP-event stage total, and every marked kernel's time.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="agg", choices=["agg", "base", "serial"])
ap.add_argument("--config", default="C2")
ap.add_argument("--events", type=int, default=0)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="", help="what the logs call the tree under --root (default: branch / parent by mode)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))

import torch  # noqa: E402

from siddhi_amd import _native as N  # noqa: E402
from siddhi_amd import compiler as C  # noqa: E402
from siddhi_amd import lowering as L  # noqa: E402
from siddhi_amd import synth  # noqa: E402

HEAD = ("define stream StockStream (id long, symbol string, price float); "
        "partition with (symbol of StockStream) begin @info(name='q') "
        "from every e1=StockStream[price>20] -> e2=StockStream[price>e1.price] within 1 sec select ")
APPS = {
    "agg": HEAD + "e1.symbol as s, count() as n, sum(e2.id) as vol, avg(e2.price - e1.price) as gain, "
                  "max(e2.price) as hi group by e1.symbol insert into M; end;",
    "base": HEAD + "e1.symbol as s, e2.id as vol, e2.price - e1.price as gain, e2.price as hi insert into M; end;",
    "serial": "define stream StockStream (id long, symbol string, price float); @info(name='q') "
              "from every e1=StockStream[price>20] -> e2=StockStream[price>e1.price] within 1 sec "
              "select sum(e2.price + 0.0) as s insert into M;",
}


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = "C1" if a.mode == "serial" else a.config
    _, events, keys, rate = synth.CONFIGS[cfg]
    n = a.events or min(events, 100_000_000)
    g = synth.generate_torch(cfg, 0, n, dev, keys=keys, rate=rate)
    key = g["key"].to(torch.int32) if a.mode != "serial" else torch.zeros(n, dtype=torch.int32, device=dev)
    cols = [g["id"], g["key"].to(torch.int32), g["price"]]
    torch.cuda.synchronize()
    app = C.parse(APPS[a.mode])
    if app.partitions:
        p = app.partitions[0]
        ctx = L.make_context(app, p.queries[0], p, {})
    else:
        ctx = L.make_context(app, app.queries[0], None, {})
    nfa = L.lower(ctx)
    opts = N.sg_options()
    opts.no_carry = 1
    h = N.Handle(N.build_desc(nfa), device=0, options=opts)
    if getattr(nfa, "aggs", None):
        h.set_aggregates(N.build_agg_desc(nfa))
    keep = []
    batch = N.make_batch(n, 0, g["ts"].data_ptr(), 0, key.data_ptr(), [c.data_ptr() for c in cols], [0] * len(cols), 1,
                         keys if app.partitions else 1, keep)
    walls, totals, kerns, matches = [], [], {}, 0
    for step in range(a.steps + 1):       # step 0 warms up (workspaces grow)
        h.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.push(batch)
        h.flush()
        wall = (time.perf_counter() - t0) * 1e3
        t = h.timing()
        matches = h.pending()
        h.discard()
        if step:
            walls.append(wall)
            totals.append(t.total_ms)
            for name, ms in t.kernels():
                kerns.setdefault(name, []).append(ms)
        print(a.mode, cfg, "warm-up" if not step else f"step {step}", f"wall {wall:.3f} ms", f"matches {matches}",
              {k: round(v, 3) for k, v in t.kernels()}, flush=True)
    h.close()
    out = {"mode": a.mode, "config": cfg, "events": n, "keys": keys, "matches": matches, "steps": a.steps,
           "tree": a.label or ("parent" if a.mode == "base" else "branch"), "push_wall_ms": statistics.median(walls),
           "stage_total_ms": statistics.median(totals),
           "kernels_ms": {k: statistics.median(v) for k, v in kerns.items()}}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
