"""Time one send_columns of N rows through the three-range app on the host route and on the device route.

    python profiles/range_route_time.py [--rows 20000000] [--reps 5] [--out FILE.json]

Host route: runtime._route_ranges (numpy masks and an np.repeat gather of every column), then GpuEngine.push of the
expanded host batch.  Device route: GpuEngine.push_ranges (sg_range_route: upload, hold kernel, scan, expand kernel),
then sg_push of the routed device batch.  Both runs use a fresh runtime per repetition, alternate in one process after
one warm-up each, and must deliver the same rows.  Reported: the wall time of the call (it ends with the matches
fetched, so the device is idle), the wall time of the routing step alone, the router's two HIP-event kernel times, and
the bytes the two kernels have to move (input columns read once, copies written once) over hold_ms + expand_ms.
Timestamps are 2 s apart (the pattern's `within` is 1 s) except one pair in a thousand, so matching and delivery stay a
small part of the call.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from siddhi_amd import QueryCallback, SiddhiManager  # noqa: E402
from siddhi_amd._native import GpuEngine  # noqa: E402

APP = ("define stream S (symbol string, price float, volume int); "
       "partition with (price>=30 as 'high' or price<30 as 'low' or price<15 as 'tiny' of S) begin @info(name='q') "
       "from every e1=S[price>10] -> e2=S[price>e1.price] within 1 sec "
       "select e1.price as p1, e2.price as p2, e2.volume as v insert into M; end;")


def columns(n, seed=1):
    rng = np.random.default_rng(seed)
    ts = np.arange(n, dtype=np.int64) * 2000
    ts[1::1000] = ts[0:-1:1000][:len(ts[1::1000])] + 1
    return dict(ts=ts, symbol=np.zeros(n, np.int32), price=np.round(rng.uniform(5, 45, n), 1).astype(np.float32),
                volume=np.arange(n, dtype=np.int32))


def one_run(cols, device_ranges):
    rt = SiddhiManager(engine=GpuEngine).createSiddhiAppRuntime(APP)
    rt.device_ranges = device_ranges
    got = []

    class CB(QueryCallback):
        def receive(self, ts, ins, rem):
            got.extend(tuple(e.data) for e in ins)

    rt.addCallback("q", CB())
    rt.start()
    eng = rt.queries[0].engine
    route = {"s": 0.0, "copies": 0}
    if device_ranges:
        inner = eng.range_router.route

        def timed(*a):
            t0 = time.perf_counter()
            r = inner(*a)          # (returns with the routed batch complete in HBM)
            route["s"] += time.perf_counter() - t0
            return r
        eng.range_router.route = timed
    else:
        inner = rt._route_ranges

        def timed(*a):
            t0 = time.perf_counter()
            r = inner(*a)
            route["s"] += time.perf_counter() - t0
            route["copies"] += r.n
            return r
        rt._route_ranges = timed
    t0 = time.perf_counter()
    rt.getInputHandler("S").send_columns(**cols)
    wall = time.perf_counter() - t0
    res = {"wall_ms": wall * 1e3, "route_ms": route["s"] * 1e3}
    if device_ranges:
        st = eng.range_router.stats()
        assert st.calls == 1
        res.update(hold_ms=st.hold_ms, expand_ms=st.expand_ms, copies=st.copies)
    else:
        assert eng.range_router.stats().calls == 0
        res.update(copies=route["copies"])
    rt.shutdown()
    return res, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    cols = columns(a.rows)
    runs = {False: [], True: []}
    want = None
    for rep in range(a.reps + 1):            # rep 0 warms both routes up
        for dev in (False, True):
            res, got = one_run(cols, dev)
            if want is None:
                want = got
            assert got == want, "the two routes delivered different rows"
            if rep:
                runs[dev].append(res)
            print(("device" if dev else "host  "), "warm-up" if not rep else f"rep {rep}",
                  {k: round(v, 3) for k, v in res.items()}, flush=True)
    med = lambda rs, k: statistics.median(r[k] for r in rs)   # noqa: E731
    copies = runs[True][0]["copies"]
    assert copies == runs[False][0]["copies"]
    # input read once: ts 8, stream 4, key 4, three 4-byte columns; per copy written: ts 8, stream 4, key 4, index 8,
    # three 4-byte columns; plus the 4-byte hold mask written and read once per row
    moved = a.rows * (8 + 4 + 4 + 12 + 8) + copies * (8 + 4 + 4 + 8 + 12)
    kernel_ms = med(runs[True], "hold_ms") + med(runs[True], "expand_ms")
    out = {"rows": a.rows, "copies": copies, "matches": len(want), "reps": a.reps,
           "host": {k: med(runs[False], k) for k in ("wall_ms", "route_ms")},
           "device": {k: med(runs[True], k) for k in ("wall_ms", "route_ms", "hold_ms", "expand_ms")},
           "bytes_moved": moved, "bytes_per_row": moved / a.rows, "kernel_gb_per_s": moved / kernel_ms / 1e6}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
