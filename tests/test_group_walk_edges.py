"""The group walker's routes and edges (csrc/gwalk.h: k_gwalk, k_gw_redo, k_gtile_count, k_gscan_project; the wide
partition in front of it, keypart.h part1_wide) on small batches with sparse key ids, row for row against the oracle.

The gate of that path is the key *bound* (`key.max() + 1`, and the engine keeps the largest bound seen), not the number
of keys: a batch of 20,000 rows in which one row carries key id 69,999 takes the wide partition and the group walker,
and the oracle (a map over the ids) does not care.  So every case here is a few 10^4 rows and every handle sees at
least one key id >= 65,536.

A push the group walker declines goes on to the tiled walker and passes parity all the same, so every case also
asserts, push by push, which route ran -- from the names of the kernels the handle timed (timing().kernels()) and
timing().spilled_units:

  WALKED          "group_walk" ran, neither "walk_count" nor "walk_record" (the tiled walker) did, and -- when the
                  oracle delivers a match for the push -- "gw_project" wrote it
  redone(k)       WALKED, "gw_redo" ran and spilled_units == k (redone(): >= 1)
  DECLINED        "group_walk" ran and "gw_project" did not: k_gwalk (or k_gw_redo) raised GW_ORDER / GW_OVERFLOW and the
                  tiled walker took the push
  DECLINED_EARLY  "gw_count" ran, "group_walk" did not, and the tiled walker's "walk_count" did: run_group_walk read the
                  partition's pack flag PK_PAY_RANGE after part1_wide and k_gw_count had run and returned before
                  launching k_gwalk
  DECLINED_WIDE   as DECLINED_EARLY, for PK_TS_RANGE: the whole push runs again with wide records
                  DECLINED and DECLINED_EARLY go on with pass 2 of the partition from the records pass 1 left, so
                  "pred" and "part_group" are each timed exactly once in such a push
  NOT_TRIED       neither "gw_count" nor "group_walk": gw_plan said no before any launch, or the partition was not the
                  wide one

A select column the lowering makes null on this shape exists (`e1[1].id`: ProjPlan kind 2, GwSel code 4) and
test_payloads covers it."""
import numpy as np
import pytest

from oracle import OracleEngine
from parity_util import assert_same, context, run_engine
from siddhi_amd.runtime import Batch, Outputs
from test_group_walk import pieces, query

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
DAY = 86_400_000
WALKED, DECLINED, DECLINED_EARLY, NOT_TRIED = "walked", "declined", "declined_early", "not_tried"
DECLINED_WIDE = "declined_wide"


def redone(k=None):
    return ("redone", k)


class _Witness:
    """GpuEngine wrapper recording, per push, the names of the kernels the handle timed and the spilled units."""
    kw = {}
    log = []

    def __init__(self, ctx):
        from siddhi_amd._native import GpuEngine
        self.e = GpuEngine(ctx, **_Witness.kw)

    def push(self, b):
        self.e.push(b)
        t = self.e.handle.timing()
        _Witness.log.append(([name for name, _ in t.kernels()], int(t.spilled_units)))

    def fetch(self):
        return self.e.fetch()

    def snapshot(self):
        return self.e.snapshot()

    def restore(self, blob):
        self.e.restore(blob)

    def close(self):
        self.e.close()


class _Oracle:
    """OracleEngine wrapper keeping every fetch apart (matches per push)."""
    outs = []

    def __init__(self, ctx):
        self.e = OracleEngine(ctx)

    def push(self, b):
        self.e.push(b)

    def fetch(self):
        o = self.e.fetch()
        _Oracle.outs.append(o)
        return o

    def close(self):
        self.e.close()


def check_route(route, names, spilled, emitted, where):
    tiled = "walk_count" in names or "walk_record" in names
    msg = f"{where}: expected {route}, kernels {names}, spilled {spilled}, oracle matches {emitted}"
    if route == WALKED or isinstance(route, tuple):
        assert "group_walk" in names and not tiled, msg
        if emitted:
            assert "gw_project" in names, msg
        if isinstance(route, tuple):
            assert "gw_redo" in names, msg
            assert spilled >= 1 if route[1] is None else spilled == route[1], msg
    elif route == DECLINED:
        assert "group_walk" in names and "gw_project" not in names, msg
    elif route in (DECLINED_EARLY, DECLINED_WIDE):
        assert "gw_count" in names and "group_walk" not in names and "gw_project" not in names and tiled, msg
    elif route == NOT_TRIED:
        assert "group_walk" not in names and "gw_count" not in names and "gw_project" not in names, msg
    else:
        raise ValueError(route)
    if route in (DECLINED, DECLINED_EARLY):
        # the tiled walker goes on from pass 1's records: the predicate pass and pass 1 of the partition ran once
        assert names.count("pred") == 1 and names.count("part_group") == 1, msg


def drive(make, q, batches, fetch_after=None, restore_after=()):
    """run_engine with a choice of the pushes after which matches are polled (default: every push) and of the pushes
    after which the state moves into a fresh handle through snapshot / restore"""
    ctx = context(q)
    eng = make(ctx)
    outs = []
    for i, b in enumerate(batches):
        eng.push(b)
        if fetch_after is None or i in fetch_after:
            outs.append(eng.fetch())
        if i in restore_after:
            blob = eng.snapshot()
            eng.close()
            eng = make(ctx)
            eng.restore(blob)
    eng.close()
    return Outputs(*[np.concatenate([getattr(o, f) for o in outs]) for f in
                     ("trigger", "ts", "key", "group", "vals", "vnull")])


def parity(q, batches, routes, min_matches=1, fetch_after=None, restore_after=(), **kw):
    """GpuEngine against the oracle over `batches`, bit for bit, and the route of every push.  Returns the oracle's
    output and its matches per fetch."""
    assert len(routes) == len(batches)
    _Oracle.outs = []
    want = drive(_Oracle, q, batches, fetch_after) if fetch_after is not None else run_engine(_Oracle, q, batches)
    per = [len(o) for o in _Oracle.outs]
    _Oracle.outs = []
    _Witness.kw, _Witness.log = kw, []
    if fetch_after is not None or restore_after:
        got = drive(_Witness, q, batches, fetch_after, restore_after)
    else:
        got = run_engine(_Witness, q, batches)
    log, _Witness.log = _Witness.log, []
    assert len(want) >= min_matches, len(want)
    assert_same(got, want)
    assert len(log) == len(batches)
    for i, (route, (names, spilled)) in enumerate(zip(routes, log)):
        emitted = per[i] if fetch_after is None else 0
        check_route(route, names, spilled, emitted, f"push {i + 1} of {len(batches)}")
    return want, per


def stock(ts, key, price, ids=None, base=0, extra=None, nulls=None):
    """rows of StockStream (id long, symbol string, price T[, volume V])"""
    n = len(key)
    key = np.asarray(key).astype(np.int32)
    ids = np.arange(base, base + n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    cols = [ids, key.copy(), np.asarray(price)] + ([] if extra is None else [np.asarray(extra)])
    return Batch(n, base, np.asarray(ts, np.int64), np.zeros(n, np.int32), key, cols,
                 [None] * len(cols) if nulls is None else nulls)


def times(n, rate=40, start=T0):
    return start + np.arange(n, dtype=np.int64) // rate


def prices(rng, n, lo=15.0, hi=38.0):
    """quarter steps: many ties"""
    return (np.round(rng.uniform(lo, hi, n) * 4) / 4).astype(np.float32)


def scattered_ids(rng, count, bound=70_001, avoid=()):
    ids = rng.choice(bound, count + len(avoid) + 8, replace=False)
    ids = ids[~np.isin(ids, np.asarray(list(avoid), np.int64))][:count]
    return np.sort(ids)


def round_robin(ids, n):
    """every id gets its rows in turn: n // len(ids) rows per key, by construction"""
    return np.asarray(ids)[np.arange(n) % len(ids)]


# ---- 1. sparse and empty groups

def sparse_batch():
    rng = np.random.default_rng(11)
    ids = np.unique(np.concatenate([rng.choice(70_001, 600, replace=False), np.arange(25_600, 25_600 + 768),
                                    [65_535, 65_536, 70_000]]))
    n = 30_000
    key = ids[rng.integers(0, len(ids), n)]
    key[0], key[1], key[-1] = 70_000, 65_536, 65_535   # the handle's first row sets the key bound: 70,001
    return stock(times(n, 20), key, prices(rng, n, 15, 40))


@pytest.mark.parametrize("cuts", [None, "rows"], ids=["one_push", "one_row_pushes"])
@pytest.mark.parametrize("cond", ["price > e1.price", "price >= e1.price", "price < e1.price", "price <= e1.price",
                                  "price > e1.price and price < 38"])
def test_sparse_and_empty_groups(cond, cuts):
    """k_gwalk over 274 groups of which ~270 hold under ten rows and many hold none (`lo == hi`: no load, no loop),
    three groups with every key active, ids 65,535 / 65,536 / 70,000 (last key of group 255, first of 256, the only
    active key of the last, partial group); as one push and cut at [1, 2, n - 1] (one-row pushes: n == 1, and every
    group but one empty while the carry holds rows).  All four operators on the monotone stack, and the scanned list
    (the PT 8, STACK=false instantiation).  Route: WALKED on every push."""
    b = sparse_batch()
    batches = [b] if cuts is None else pieces(b, [1, 2, b.n - 1])
    want, _ = parity(query(cond), batches, [WALKED] * len(batches))
    assert len(want) > 1000


# ---- 2. key-bound edges of the wide partition

def lbs_of(kb):
    """part1_wide's supergroup shift: the smallest with at most 64 supergroups of 2^lbs groups"""
    ng, lbs = (kb + 255) >> 8, 0
    while ((ng + (1 << lbs) - 1) >> lbs) > 64 and lbs < 8:
        lbs += 1
    return lbs


@pytest.mark.parametrize("kb", [65_537, 65_792, 65_793, 131_072, 131_073, 1_048_575, 1_048_576, 1_048_577])
def test_key_bound_edges(kb):
    """part1_wide's two counting passes (k_hist_wide, k_part1 over supergroups, k_part1b) where its plan changes: the
    first bound past the two-pass LDS partition (65,537: 257 groups, one key in the last), a bound that fills its last
    group and one that starts a new one (65,792 / 65,793), the supergroup shift going from 3 to 4 (131,072: 512 groups;
    131,073: 513), and the largest bound of the path (1,048,576 = 4096 groups; 1,048,575 leaves the last key out).
    The same 20,000 rows every time; only the top id moves, with the first key of the last group and the first and
    last keys of the last supergroup's first group.  Route: WALKED; 1,048,577 is past the gate: NOT_TRIED (radix sort)."""
    rng = np.random.default_rng(5)
    n = 20_000
    ids = scattered_ids(rng, 800, bound=60_000)
    key = ids[rng.integers(0, len(ids), n)]
    top = kb - 1
    g_last = top >> 8
    g_first = (g_last >> lbs_of(kb)) << lbs_of(kb)
    special = sorted(k for k in {top, g_last << 8, g_first << 8, (g_first << 8) + 255} if k < kb)
    for j, s in enumerate(special):
        key[100 + 7 * j + 40 * np.arange(12)] = s
    assert key.max() + 1 == kb
    b = stock(times(n, 20), key, prices(rng, n, 15, 40))
    want, _ = parity(query(), [b], [WALKED if kb <= 1_048_576 else NOT_TRIED])
    assert len(want) > 1000
    assert np.isin(np.asarray(special), want.key).all()   # every placed key delivers


# ---- 3. chunk edges

def chunk_batch(pt, lanes):
    """five groups with exactly 256*pt - 1, 256*pt, 256*pt + 1, 2*256*pt and 2*256*pt + 1 rows, their rows spread over
    the in-group keys `lanes`, interleaved with each other and with 2,000 rows of scattered keys; in the last two, one
    key holds a six-deep falling run across the first chunk boundary and a spike 40 rows after it"""
    rng = np.random.default_rng(100 + pt + len(lanes))
    c = 256 * pt
    counts = [c - 1, c, c + 1, 2 * c, 2 * c + 1]
    groups = [258, 260, 262, 264, 266]
    label = np.concatenate([np.full(m, j) for j, m in enumerate(counts)] + [np.full(2_000, -1)])
    rng.shuffle(label)
    n = len(label)
    key = np.empty(n, np.int64)
    price = prices(rng, n)
    bg = scattered_ids(rng, 400, bound=65_536)
    key[label < 0] = bg[rng.integers(0, len(bg), int((label < 0).sum()))]
    run_lane = lanes[len(lanes) // 2]
    for j, (g, m) in enumerate(zip(groups, counts)):
        at = np.nonzero(label == j)[0]               # the group's rows in arrival order
        assert len(at) == m
        key[at] = (g << 8) + np.asarray(lanes)[rng.integers(0, len(lanes), m)]
        if m >= 2 * c:
            run = at[c - 3:c + 3]                    # group rows c-3 .. c+2: three each side of the chunk boundary
            key[run] = (g << 8) + run_lane
            price[run] = np.float32(39.5) - np.arange(6, dtype=np.float32) * np.float32(0.25)
            key[at[c + 40]] = (g << 8) + run_lane
            price[at[c + 40]] = np.float32(39.75)
    return stock(times(n, 40), key, price), [(g << 8) + run_lane for g in groups[3:]]


@pytest.mark.parametrize("lanes", [list(range(256)), [0, 17, 255]], ids=["256_keys", "3_keys"])
@pytest.mark.parametrize("pt,ring,env", [(6, 0, None), (8, 8, None), (4, 32, None), (10, 0, "10"), (12, 0, "12")])
def test_chunk_edges(pt, ring, env, lanes, monkeypatch):
    """k_gwalk<PT>'s chunk loop where the group's row count meets the chunk (256 * PT rows): the `load` tail clamp
    (`rows - 1` re-read), the masked tail of the counting sort and the `base + ROWS < hi` prefetch guard, at one row
    under, exactly, and one row over one and two chunks.  Every instantiation: PT 6 (default ring 16), PT 8 (ring 8),
    PT 4 (ring 32: the cap == 32 kernel) and, through SG_DEBUG_GW_PT, PT 10 and 12.  Rows over all 256 keys of the group,
    then over 3 (runs of hundreds of rows per lane inside one chunk).  A falling run across the chunk boundary keeps
    one lane's ring and match-area cursor alive from chunk to chunk; its spike must deliver all six.  One first push,
    so no carry.  Route: WALKED (a lane that outgrows a small ring is redone, which is still the group walker)."""
    if env is not None:
        monkeypatch.setenv("SG_DEBUG_GW_PT", env)
    b, run_keys = chunk_batch(pt, lanes)
    want, _ = parity(query(), [b], [WALKED], ring_cap=ring)
    assert len(want) > 1000
    for k in run_keys:   # the spike's trigger delivers the six partials of the run, oldest first
        m = want.key == k
        p1 = (want.vals[m, 2] & 0xffffffff).astype(np.uint32).view(np.float32)
        p2 = (want.vals[m, 3] & 0xffffffff).astype(np.uint32).view(np.float32)
        assert (p1[p2 == np.float32(39.75)][:6] == np.float32(39.5) - np.arange(6, dtype=np.float32) * np.float32(0.25)).all()


# ---- 4. redo

SMALL = [66_000, 66_001, 300]     # two keys of one group and one of another
BIG = [66_100, 67_000]            # keys of more than GW_REDO_LDS rows
CUT = 3_450


def redo_stream(small, big, cap=16):
    """20,000 rows, ten per key over 2,000 scattered keys in turn (no such key can hold more than ten partials), in
    which every key of `small` and `big` gets a strictly falling run of cap + 1 candidates and then a price above all
    of them, at rows 3000 + j + 50 i: run rows 0..8 lie before row CUT, the rest and the spike after.  A key of `big`
    also gets 12 rows of rising price before the cut (each completes the one before it, from the key's very first row
    on; the run's first row completes the last) and 2,280 rows after it (non-candidates up to the spike)."""
    rng = np.random.default_rng(41)
    n = 20_000
    bg = scattered_ids(rng, 2_000, avoid=SMALL + BIG)
    key = round_robin(bg, n).astype(np.int64)
    price = prices(rng, n)
    taken = np.zeros(n, bool)
    for j, k in enumerate(list(small) + list(big)):
        run = 3_000 + j + 50 * np.arange(cap + 2)
        key[run] = k
        price[run[:-1]] = np.float32(39.5) - np.arange(cap + 1, dtype=np.float32) * np.float32(0.25)
        price[run[-1]] = np.float32(39.9)
        taken[run] = True
    for k in big:
        free = np.nonzero(~taken[:CUT])[0]
        pre = np.sort(rng.choice(free, 12, replace=False))
        key[pre], price[pre], taken[pre] = k, np.float32(21) + np.arange(12, dtype=np.float32), True
        free = CUT + np.nonzero(~taken[CUT:])[0]
        post = rng.choice(free, 2_280, replace=False)
        key[post], taken[post] = k, True
        price[post[post < 3_900]] = np.float32(15)   # (nothing between the rows of the run completes part of it)
    return stock(times(n, 40), key, price)


def test_redo_lds_branch():
    """k_gw_redo with the key's records and list in LDS (nk <= GW_REDO_LDS): three keys whose list outgrows the default
    ring (16) by construction, two of them lanes of one workgroup (both stop, both are listed, the other 254 lanes of
    the group are not).  Route: redone(3)."""
    parity(query(), [redo_stream(SMALL, [])], [redone(3)], min_matches=1000)


def test_redo_hbm_branch():
    """k_gw_redo's HBM branch (nk > GW_REDO_LDS = 2048: records read through `rows`, the list in the hv / ht / hp planes
    at the key's own offset `kb`): two keys of 2,310 rows each, walked by two workgroups at once.  Route: redone(2)."""
    b = redo_stream([], BIG)
    assert all(int((b.key == k).sum()) > 2_048 for k in BIG)
    parity(query(), [b], [redone(2)], min_matches=1000)


def test_redo_run_cut_by_push_boundary():
    """both redo branches with the falling run cut by the push boundary: push 1 leaves nine partials per key in the ring
    (no overflow: WALKED), push 2 replays them as carried rows and the run's other eight outgrow the ring -- the redo
    walks carried rows (`r < a.nc`: complete, never emit) and must deliver nothing twice.  The two big keys have 2,280
    rows plus their carried ones in push 2 (HBM branch).  Routes: WALKED, redone(5)."""
    b = redo_stream(SMALL, BIG)
    assert all(int((b.key[CUT:] == k).sum()) > 2_048 for k in BIG)
    parity(query(), pieces(b, [CUT]), [WALKED, redone(5)], min_matches=1000)


@pytest.mark.parametrize("nover", [65_536, 65_537])
def test_redo_list_boundary(nover):
    """the `o < a.ovf_cap` boundary of k_gwalk's overflow list (ovf_cap = min(kb, 65536)): ring_cap 2, 70,000 keys in
    turn -- price 39, then 38, then 37 for the first `nover` keys only, then 39.5 for every key.  Three falling
    candidates outgrow a ring of two, two do not: exactly `nover` keys overflow.  65,536 fill the list: redone(65536).
    65,537 raise GW_OVERFLOW and the whole push runs on the tiled walker: DECLINED.  Either way every key's spike
    completes all its partials: 2 * 70,000 + nover matches."""
    kb = 70_000
    allk = np.arange(kb)
    key = np.concatenate([allk, allk, allk[:nover], allk])
    price = np.concatenate([np.full(kb, 39.0), np.full(kb, 38.0), np.full(nover, 37.0), np.full(kb, 39.5)]).astype(np.float32)
    b = stock(times(len(key), 1000), key, price)
    assert b.n == 3 * kb + nover
    want, _ = parity(query(), [b], [redone(65_536) if nover == 65_536 else DECLINED], ring_cap=2)
    assert len(want) == 2 * kb + nover


# ---- 5. projection

SELECTS = {1: "e1.id as a",
           3: "e2.price as a, e1.id as b, e1.price as c",
           5: "e1.id as a, e2.id as b, e1.price as c, e2.price as d, e1.id as e"}
DEEP = [66_200, 100]


def projection_stream():
    """the ten-rows-per-key background, and two keys with a 300-deep falling run each (rows 2000 + j + 20 i) whose
    spikes are rows 9000 and 9001: two triggers of 300 matches in one 256-row tile"""
    rng = np.random.default_rng(43)
    n = 20_000
    bg = scattered_ids(rng, 2_000, avoid=DEEP)
    key = round_robin(bg, n).astype(np.int64)
    price = prices(rng, n)
    for j, k in enumerate(DEEP):
        run = 2_000 + j + 20 * np.arange(300)
        key[run] = k
        price[run] = np.float32(39.5) - np.arange(300, dtype=np.float32) * np.float32(0.05)
        key[9_000 + j] = k
        price[9_000 + j] = np.float32(39.9)
    return stock(times(n, 40), key, price)


@pytest.mark.parametrize("nsel", [1, 3, 5])
def test_projection_select_counts(nsel):
    """k_gscan_project with 1, 3 and 5 select columns from the four sources the walker accepts (e1 payload, e1 value,
    e2 value, e2 payload).  The record stride 32 + 8 * nsel is 8 mod 16 for an odd count, so a tile whose first output
    slot is odd stores through the 8-byte branch, and one that ends on an odd slot ends on a half 16-byte word.  Rows
    9000 and 9001 deliver 300 matches each: a trigger of more than GW_PROJ_S (256) matches, a tile of more than 512, so
    the staging runs in three rounds and both triggers straddle a round.  k_gtile_count's tile sums feed the bases.
    Route: redone(2) (the two deep keys, LDS branch)."""
    want, _ = parity(query(select=SELECTS[nsel]), [projection_stream()], [redone(2)], min_matches=1000)
    assert int((want.trigger == 9_000).sum()) == 300 and int((want.trigger == 9_001).sum()) == 300


@pytest.mark.parametrize("nsel", [1, 3, 5])
def test_projection_poll_once_after_two_pushes(nsel):
    """two pushes, one poll: the second push's k_gscan_project writes at out_base != 0 behind the first push's records.
    The first push delivers an odd number of matches (asserted), so with an odd select count the second push's first
    tile starts on an 8-byte boundary.  The oracle is driven the same way.  Routes: redone(2) (both deep runs lie in
    push 1), redone(1) (the second key's 300 carried partials outgrow the ring again)."""
    b = projection_stream()
    batches = pieces(b, [9_001])
    first = run_engine(OracleEngine, query(select=SELECTS[nsel]), batches[:1])
    assert len(first) % 2 == 1
    parity(query(select=SELECTS[nsel]), batches, [redone(2), redone(1)], min_matches=1000, fetch_after=[1])


# ---- 6. values

def vquery(ptype, vtype, cond, select):
    return (f"define stream StockStream (id long, symbol string, price {ptype}, volume {vtype}); "
            "partition with (symbol of StockStream) begin @info(name='q') "
            f"from every e1=StockStream[price > -100] -> e2=StockStream[{cond}] within 1 sec "
            f"select {select} insert into M; end;")


FLOAT_POOL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.0, 1.0, 1.0, -1.0, -1.0, 2.5, 2.5, -99.5,
                       -100.0, -150.0, 3e38, -3e38], np.float32)


def value_batch(ptype, seed=7, ids=None, volume=None):
    rng = np.random.default_rng(seed)
    n = 20_000
    keys = scattered_ids(rng, 1_500)
    key = keys[rng.integers(0, len(keys), n)]
    key[0] = 70_000
    if ptype == "float":
        price = FLOAT_POOL[rng.integers(0, len(FLOAT_POOL), n)]
    else:
        price = rng.integers(-50, 51, n).astype(np.int32)
    if volume is None:
        volume = rng.integers(0, 1000, n).astype(np.int32)
    return stock(times(n, 20), key, price, ids=ids, extra=volume)


@pytest.mark.parametrize("op", [">", ">=", "<", "<="])
@pytest.mark.parametrize("ptype", ["float", "int"])
def test_compared_values(ptype, op):
    """the 32-bit value word of the walker record and of the match area (val_bits, cmp_op, is_nan_val; the projection's
    wid(bits, vfloat): FLOAT bits zero-extended, INT sign-extended).  FLOAT from a pool of NaN (never a candidate,
    completes nothing), +-inf, +-0.0 (equal, different bits), denormals, +-3e38 and many ties, behind an A filter that
    admits negatives; INT in [-50, 50].  Route: WALKED."""
    q = vquery(ptype, "int", f"price {op} e1.price", "e1.id as id1, e2.id as id2, e1.price as p1, e2.price as p2")
    want, _ = parity(q, [value_batch(ptype)], [WALKED], min_matches=1000)
    if ptype == "int":
        assert (want.vals[:, 2] < 0).any() and (want.vals[:, 3] < 0).any()


@pytest.mark.parametrize("case", ["negative_long", "negative_int", "float", "null_select"])
def test_payloads(case):
    """the 32-bit payload word: a negative LONG id and a negative INT column (sign-extended by k_gscan_project and by the
    carry), a FLOAT column (GwArgs.pzero: zero-extended bits, -0.0 and NaN among them), and a select column the lowering
    makes null (`e1[1].id`: GwSel code 4, bit set in the record's null mask).  Two pushes, so the carried payloads are
    read back.  Route: WALKED."""
    rng = np.random.default_rng(8)
    n = 20_000
    ids = volume = None
    vtype = "int"
    if case == "negative_long":
        ids, sel = -5_000_000 + 3 * np.arange(n, dtype=np.int64), "e1.id as a, e2.id as b, e1.price as c"
    elif case == "negative_int":
        volume, sel = rng.integers(-2_000_000_000, 1000, n).astype(np.int32), "e1.volume as a, e2.price as b, e2.volume as c"
    elif case == "float":
        vtype = "float"
        volume = FLOAT_POOL[rng.integers(0, len(FLOAT_POOL), n)]
        sel = "e1.volume as a, e2.volume as b, e1.price as c"
    else:
        sel = "e1[1].id as z, e1.id as a, e2.price as b"
    b = value_batch("float", seed=9, ids=ids, volume=volume)
    want, _ = parity(vquery("float", vtype, "price > e1.price", sel), pieces(b, [8_000]), [WALKED, WALKED], min_matches=1000)
    if case == "null_select":
        assert want.vnull[:, 0].all() and not want.vnull[:, 1:].any()
    elif case != "float":
        assert (want.vals[:, 0] < 0).any()


# ---- 7. the `within` edge

@pytest.mark.parametrize("cuts", [None, [1, 2, 3, 4]], ids=["one_push", "one_row_pushes"])
def test_within_edge_literal(cuts):
    """GwLane::step's lazy expiry `(uint32_t)(dts - hts) > wi` at the edge, one key: a partial exactly `within` old
    completes, one a millisecond older is dropped.  Rows (ms, price): (0, 30) (1000, 31) (5000, 25) (6001, 35)
    (7001, 36).  Row 1 completes row 0 (exactly 1000 ms); row 3 comes 1001 ms after row 2: nothing; row 4 completes row
    3.  As one push, and row by row (the carried partial expires on a later push).  Route: WALKED."""
    ts = T0 + np.array([0, 1000, 5000, 6001, 7001], np.int64)
    price = np.array([30, 31, 25, 35, 36], np.float32)
    b = stock(ts, np.full(5, 66_000), price)
    batches = [b] if cuts is None else pieces(b, cuts)
    want, _ = parity(query(), batches, [WALKED] * len(batches), min_matches=2)
    assert want.trigger.tolist() == [1, 4]
    assert want.ts.tolist() == [T0 + 1000, T0 + 7001]
    assert want.key.tolist() == [66_000, 66_000]
    assert want.vals[:, :2].tolist() == [[0, 1], [3, 4]]
    bits = lambda x: int(np.float32(x).view(np.uint32))
    assert want.vals[:, 2:].tolist() == [[bits(30), bits(31)], [bits(35), bits(36)]]


@pytest.mark.parametrize("within,gap_days,kept", [("20 days", 19, True), ("30 days", 19, True), ("60 days", 19, True),
                                                   ("20 days", 21, False)])
def test_within_days(within, gap_days, kept):
    """`within` near and past the 32-bit word GwLane compares it in (wi = min(within, 2^32 - 1)): 20 days fits 31 bits,
    30 days needs 32, 60 days is clamped.  Two pushes 19 days apart (the carried rows' offsets still fit the record's
    31 bits): partials of push 1 complete in push 2.  With 20 days and a gap of 21 every carried partial expires on its
    key's first row.  The oracle's own output shows which happened, so neither case passes empty.  ring_cap=16 is
    forced: the ring gw_plan would size from such a window is past its limit of 32 and the push would not be tried.
    Routes: WALKED, WALKED."""
    rng = np.random.default_rng(13)
    n = 10_000
    keys = scattered_ids(rng, 1_000)
    b1 = stock(times(n, 40), round_robin(keys, n), prices(rng, n, 15, 40))
    b2 = stock(times(n, 40, T0 + gap_days * DAY), round_robin(keys, n), prices(rng, n, 15, 40), base=n)
    q = query().replace("within 1 sec", "within " + within)
    want, per = parity(q, [b1, b2], [WALKED, WALKED], min_matches=1000, ring_cap=16)
    second = want.vals[per[0]:, 0]
    assert per[1] > 1000
    assert bool((second < n).any()) == kept
    if kept:
        assert int((second < n).sum()) > 500


# ---- 8. declines after launch

def ordinary(rng, keys, n, start, base, ids=None):
    return stock(times(n, 40, start), round_robin(keys, n), prices(rng, n, 15, 40), ids=ids, base=base)


def test_decline_payload_past_32_bits():
    """PK_PAY_RANGE raised by the partition after part1_wide and k_gw_count have run: ids reach 2^31 - 5,001 in push 1
    (WALKED, partials carried as 32-bit payloads) and pass 2^31 in push 2, which run_group_walk hands to the tiled walker
    (e1 gathered by row) before k_gwalk is launched: DECLINED_EARLY.  The carry of push 1 must be intact: push 2
    delivers matches whose e1 is of push 1.  Push 2 ends with one row per key of price 1000 and a small id, which
    completes every partial, so what push 3 finds carried fits 32 bits again: WALKED."""
    rng = np.random.default_rng(17)
    n = 20_000
    keys = scattered_ids(rng, 1_500)
    hi = (1 << 31) - 5_001
    b1 = ordinary(rng, keys, n, T0, 0, ids=hi - (n - 1) + np.arange(n, dtype=np.int64))
    b2 = ordinary(rng, keys, n, T0 + 500, n, ids=hi + 1 + np.arange(n, dtype=np.int64))
    b2.cols[2][-len(keys):] = np.float32(1000)
    b2.cols[0][-len(keys):] = np.arange(len(keys))
    b3 = ordinary(rng, keys, n, T0 + 1000, 2 * n, ids=10_000 + np.arange(n, dtype=np.int64))
    want, per = parity(query(), [b1, b2, b3], [WALKED, DECLINED_EARLY, WALKED], min_matches=10_000)
    e1 = want.vals[per[0]:per[0] + per[1], 0]
    assert (e1 <= hi).any() and (e1 >= 1 << 31).any()
    assert int(want.vals[:, 0].max()) > (1 << 31) + 10_000


def test_decline_time_span_past_31_bits():
    """PK_TS_RANGE (run_group_walk returns 2: wide records): push 2 comes 30 days after push 1, so its first carried row
    lies more than 2^31 ms before its rows.  The code reads the pack flags before it launches k_gwalk, so "group_walk"
    is absent while "gw_count" ran: DECLINED_WIDE, on every run.  Every key gets rows in push 2, which drops its
    30-day-old partials; push 3 follows at once: WALKED."""
    rng = np.random.default_rng(19)
    n = 20_000
    keys = scattered_ids(rng, 1_500)
    b1 = ordinary(rng, keys, n, T0, 0)
    b2 = ordinary(rng, keys, n, T0 + 30 * DAY, n)
    b3 = ordinary(rng, keys, n, T0 + 30 * DAY + 500, 2 * n)
    want, per = parity(query(), [b1, b2, b3], [WALKED, DECLINED_WIDE, WALKED], min_matches=10_000)
    assert per[2] > 1000 and (want.vals[per[0] + per[1]:, 0] < 2 * n).any()   # push 3 completes partials of push 2


def test_decline_time_goes_back():
    """GW_ORDER after a walked push: push 1 is WALKED and hands its partials on as value rows; in push 2 key 66,010 gets
    rows at +100 ms (30), +50 ms (25: its time goes back) and +200 ms (50), so k_gwalk raises GW_ORDER after it has
    written trigger words and matches: DECLINED, and the tiled path walks that key exactly over the value carry.  The
    row of price 50 completes both, so the key's carried list (one partial) is in time order again, and by
    EveryNextState's rule -- the carry is each key's final pending list, nothing else is remembered about a key --
    push 3 is WALKED; there the key's row of price 60 completes the partial of push 2."""
    rng = np.random.default_rng(23)
    n = 20_000
    keys = scattered_ids(rng, 1_500, avoid=[66_010])
    b1 = ordinary(rng, keys, n, T0, 0)
    b2 = ordinary(rng, keys, n, T0 + 500, n)
    b3 = ordinary(rng, keys, n, T0 + 1000, 2 * n)
    for row, dt, p in [(4_000, 100, 30), (4_001, 50, 25), (8_000, 200, 50)]:
        b2.key[row] = b2.cols[1][row] = 66_010
        b2.ts[row] = T0 + 500 + dt
        b2.cols[2][row] = np.float32(p)
    b1.key[5] = b1.cols[1][5] = 66_010
    b1.cols[2][5] = np.float32(45)                   # a partial of push 1 the rows of push 2 do not complete
    b3.key[100] = b3.cols[1][100] = 66_010
    b3.cols[2][100] = np.float32(60)
    want, per = parity(query(), [b1, b2, b3], [WALKED, DECLINED, WALKED], min_matches=10_000)
    m = want.key == 66_010
    assert want.vals[m, :2].tolist() == [[5, n + 8_000], [n + 4_000, n + 8_000], [n + 4_001, n + 8_000],
                                         [n + 8_000, 2 * n + 100]]


def test_null_mask_is_not_tried():
    """a null mask on a column (here the compared one) makes gw_plan return before any launch: NOT_TRIED for push 2,
    which runs on the tiled walker over the value carry of push 1 (WALKED); push 3 has no mask: WALKED."""
    rng = np.random.default_rng(29)
    n = 20_000
    keys = scattered_ids(rng, 1_500)
    b1 = ordinary(rng, keys, n, T0, 0)
    b2 = ordinary(rng, keys, n, T0 + 500, n)
    b3 = ordinary(rng, keys, n, T0 + 1000, 2 * n)
    b2.nulls[2] = (rng.random(n) < 0.05).astype(np.uint8)
    want, per = parity(query(), [b1, b2, b3], [WALKED, NOT_TRIED, WALKED], min_matches=10_000)
    assert (want.vals[per[0]:per[0] + per[1], 0] < n).any()


# ---- 9. growing past 65,536 keys mid-stream

@pytest.mark.parametrize("restore", [False, True], ids=["one_handle", "snapshot_restore"])
def test_growing_past_65536_keys(restore):
    """how every real stream of the path begins: push 1 has a key bound of 60,000 (the two-pass LDS partition and the
    tiled walker: NOT_TRIED) and leaves partials carried as rows; push 2 brings id 65,536 and is WALKED over that
    carry; push 3 is WALKED.  Again with the state moved into a fresh handle by snapshot / restore after pushes 1 and
    2 (pushes 2 and 3 both hold an id past 65,535, so the route does not hang on the restored key bound)."""
    rng = np.random.default_rng(31)
    n = 20_000
    keys = scattered_ids(rng, 1_500, bound=59_999)
    keys[-1] = 59_999
    b1 = ordinary(rng, keys, n, T0, 0)
    more = np.concatenate([keys, [65_536, 66_000]])
    b2 = ordinary(rng, more, n, T0 + 500, n)
    b3 = ordinary(rng, more, n, T0 + 1000, 2 * n)
    assert b1.key.max() + 1 == 60_000
    want, per = parity(query(), [b1, b2, b3], [NOT_TRIED, WALKED, WALKED], min_matches=10_000,
                       restore_after=(0, 1) if restore else ())
    assert (want.vals[per[0]:per[0] + per[1], 0] < n).any()   # push 2 completes partials of push 1
