"""The wide partition's coarse group table and the one-kernel key bases (csrc/keypart.h: k_hist_wide, part1_wide,
k_part1b, part2_range; csrc/gwalk.h: k_gw_count), row for row against the oracle, with the route of every push asserted
as in test_group_walk_edges.

The group table o1 has one column per W = 8 pass-1 segments (P1_COL_SEGS), and the pass-1b and pass-2 segment sizes
(tsb, ts2) are multiples of W, so every reader lands on a column.  The plan of a push of nt virtual rows (carried rows
included) under a key bound kb > 65,536, restated in `plan` below and asserted by the cases:

  seg1 = 1024 * clamp(nt // 2^21, 1, 32)        rows per pass-1 segment (1024 for every push under 4M rows)
  ns1  = ceil(nt / seg1)                        pass-1 segments: the supergroup table's columns
  nc1  = ceil(ns1 / W)                          the group table's columns
  ng   = ceil(kb / 256), lbs = the smallest shift with ceil(ng / 2^lbs) <= 64, nsg = ceil(kb / 2^(8 + lbs))
  nsb  = clamp((nt // nsg) // P1B_ROWS, 1, ns1); tsb = ceil(ns1 / nsb) rounded up to a multiple of W; nsb = ceil(ns1 / tsb)
  ts2  = clamp(8 * ng, 1, ns1) (seg1 = 1024) rounded up to a multiple of W; nj = ceil(ns1 / ts2)

P1B_ROWS is 32,768, or SG_DEBUG_P1B_ROWS (a test hook: several pass-1b segments in a push of a few 10^4 rows)."""
import numpy as np
import pytest

import test_group_walk_edges as edges
from test_group_walk import query
from test_group_walk_edges import (DECLINED, T0, WALKED, ordinary, parity, prices, redone, scattered_ids, stock, times)

pytestmark = pytest.mark.gpu

W = 8
SEG1 = 1024


def plan(kb, nt, p1b_rows=32_768):
    seg1 = 1024 * max(1, min(32, nt // (1 << 21)))
    ns1 = max(1, -(-nt // seg1))
    ng, lbs = (kb + 255) >> 8, 0
    while ((ng + (1 << lbs) - 1) >> lbs) > 64 and lbs < 8:
        lbs += 1
    nsg = (kb + (1 << (8 + lbs)) - 1) >> (8 + lbs)
    nsb = max(1, min(ns1, max(1, nt // nsg) // p1b_rows))
    tsb = -(-(-(-ns1 // nsb)) // W) * W
    nsb = -(-ns1 // tsb)
    ts2 = max(1, min(ns1, 8192 * ng // seg1))
    ts2 = -(-ts2 // W) * W
    return dict(seg1=seg1, ns1=ns1, nc1=-(-ns1 // W), ng=ng, lbs=lbs, nsg=nsg, nsb=nsb, tsb=tsb, ts2=ts2,
                nj=-(-ns1 // ts2))


def spy_routes(monkeypatch):
    """the kernel names of every push parity() checks"""
    seen = []
    real = edges.check_route

    def spy(route, names, spilled, emitted, where):
        seen.append(list(names))
        real(route, names, spilled, emitted, where)

    monkeypatch.setattr(edges, "check_route", spy)
    return seen


def go_back(b, start, key=66_010):
    """key `key` gets rows at +100 ms, +50 ms (its time goes back: GW_ORDER) and +200 ms; the last completes both"""
    for row, dt, p in [(4_000, 100, 30), (4_001, 50, 25), (8_000, 200, 50)]:
        b.key[row] = b.cols[1][row] = key
        b.ts[row] = start + dt
        b.cols[2][row] = np.float32(p)


# ---- 1, 3. several columns with a ragged tail; the same push declined

def ragged_pushes(seed):
    rng = np.random.default_rng(seed)
    n = 40_000
    keys = scattered_ids(rng, 1_500, avoid=[66_010])
    keys[-1] = 70_000
    sgs = np.unique(keys >> 11)
    assert len(sgs) >= 3 and sgs[-1] == 34           # rows in the last, partial supergroup (groups 272 and 273 of 274)
    p = plan(70_001, n, 256)
    assert (p["ns1"], p["nc1"], p["nsg"], p["tsb"], p["nsb"], p["ts2"], p["nj"]) == (40, 5, 35, 16, 3, 40, 1)
    return [ordinary(rng, keys, n, T0, 0), ordinary(rng, keys, n, T0 + 1000, n)]


def test_several_columns_ragged_tail(monkeypatch):
    """Two pushes of 40,000 rows, key bound 70,001, SG_DEBUG_P1B_ROWS=256: ng = 274, lbs = 3, nsg = 35; push 1 has
    nt = 40,000, seg1 = 1024, ns1 = 40 (the last segment holds 64 rows), W = 8, nc1 = 5; nsb = (40,000 // 35) // 256 = 4,
    tsb = 10 -> 16, nsb = 3: k_part1b reads o1 at columns 0, 2 and 4, and its last segment covers 8 of 16 pass-1
    segments (ns1 is no multiple of tsb); ts2 = 40, nj = 1.  Push 2 has the pending lists of push 1 as carried virtual
    rows in front (nt = nc + 40,000: ns1 of 41 or more, nc1 = 6, the last column ragged).  1,500 scattered keys in
    every supergroup, the last, partial one (ids from 69,632) included.  Route: WALKED, WALKED."""
    monkeypatch.setenv("SG_DEBUG_P1B_ROWS", "256")
    want, per = parity(query(), ragged_pushes(3), [WALKED, WALKED], min_matches=10_000)
    assert (want.vals[per[0]:, 0] < 40_000).any()    # push 2 completes partials of push 1: the carry was in front


def test_declined_push_reads_coarse_table(monkeypatch):
    """The shape of test_several_columns_ragged_tail (ns1 = 40, W = 8, nc1 = 5, tsb = 16, nsb = 3, ts2 = 40, nj = 1 in
    push 1; push 2 behind its carried rows), and in push 2 key 66,010's time goes back: k_gwalk raises GW_ORDER, and
    pass 2 of the partition (k_part2_hist, k_part2 through part2_range) goes on from the coarse o1 that part1_wide left.
    Route: WALKED, DECLINED; the declined push ran the tiled walker's walk_count, and pred and part_group once each."""
    monkeypatch.setenv("SG_DEBUG_P1B_ROWS", "256")
    seen = spy_routes(monkeypatch)
    b1, b2 = ragged_pushes(3)
    go_back(b2, T0 + 1000)
    parity(query(), [b1, b2], [WALKED, DECLINED], min_matches=10_000)
    names = seen[1]
    assert "gw_count" in names and "walk_count" in names
    assert names.count("pred") == 1 and names.count("part_group") == 1 and names.count("part_hist") == 1


# ---- 2. column edges

def edge_batch(n, seed=0, base=0, start=T0):
    """n rows over 40 keys of groups 3, 4, 130, 131 and 273 only: supergroups 0, 16 and 34 of 35 hold rows, every other
    supergroup and every other group is empty"""
    rng = np.random.default_rng(50 + seed)
    ids = np.concatenate([(g << 8) + rng.choice(256, 8, replace=False) for g in (3, 4, 130, 131)] +
                         [(273 << 8) + np.array([0, 1, 5, 50, 60, 100, 111, 112])])
    key = ids[rng.integers(0, len(ids), n)]
    key[0] = 70_000
    return stock(times(n, 40, start), key, prices(rng, n, 15, 40), base=base)


@pytest.mark.parametrize("n", [1, 1_000, 1_024, W * SEG1 - 1, W * SEG1, W * SEG1 + 1])
def test_column_edges_one_push(n, monkeypatch):
    """One push of n rows, key bound 70,001 (ng = 274, nsg = 35), seg1 = 1024, SG_DEBUG_P1B_ROWS=64; rows in three of
    the 35 supergroups and five of the 274 groups, all others empty.  n = 1: one row (ns1 = nc1 = 1, no match);
    n = 1,000 and 1,024: exactly one pass-1 segment (ns1 = 1, nc1 = 1, tsb = 8, nsb = 1, ts2 = 8, nj = 1), not full and
    full; n = 8,191 and 8,192 = W * seg1: one whole column (ns1 = 8, nc1 = 1, tsb = 8, nsb = 1), its last segment one row
    short and full; n = 8,193: one row in a second column (ns1 = 9, nc1 = 2; nsb = (8,193 // 35) // 64 = 3, tsb = 3 -> 8,
    nsb = 2: k_part1b's second segment reads column 1 and covers that one row).  Route: WALKED."""
    monkeypatch.setenv("SG_DEBUG_P1B_ROWS", "64")
    p = plan(70_001, n, 64)
    want = {1: (1, 1, 1), 1_000: (1, 1, 1), 1_024: (1, 1, 1), 8_191: (8, 1, 1), 8_192: (8, 1, 1), 8_193: (9, 2, 2)}[n]
    assert (p["ns1"], p["nc1"], p["nsb"]) == want and p["tsb"] == 8 and p["nj"] == 1
    parity(query(), [edge_batch(n)], [WALKED], min_matches=0 if n == 1 else 100)


def test_column_edges_carried(monkeypatch):
    """The same edges with state carried: pushes of 8,192, 1, 8,191 and 8,193 rows on one handle (nt = nc + n, so the
    carried rows shift every edge by the pending lists' size: a one-row push whose other virtual rows are all carried,
    and columns whose first rows are carried ones).  Plans as in test_column_edges_one_push, ns1 <= 10.
    Route: WALKED on every push."""
    monkeypatch.setenv("SG_DEBUG_P1B_ROWS", "64")
    sizes, batches, base = [W * SEG1, 1, W * SEG1 - 1, W * SEG1 + 1], [], 0
    for i, n in enumerate(sizes):
        batches.append(edge_batch(n, seed=i, base=base, start=T0 + 250 * i))
        base += n
    want, per = parity(query(), batches, [WALKED] * 4, min_matches=1_000)
    assert (want.vals[per[0]:, 0] < W * SEG1).any()   # a later push completes partials of push 1


# ---- 4. the natural plan

@pytest.mark.timeout(300)
@pytest.mark.parametrize("route", [WALKED, DECLINED])
def test_natural_plan_two_columns_per_segment(route, monkeypatch):
    """No hook: 2,300,000 rows over 2,000 keys, key bound 65,700 (ng = 257, lbs = 3, nsg = 33): seg1 = 1024, ns1 = 2,247,
    W = 8, nc1 = 281; nsb = (2,300,000 // 33) // 32,768 = 2, tsb = 1,124 -> 1,128, nsb = 2 (k_part1b reads columns 0 and
    141); ts2 = 8 * 257 = 2,056 (a multiple of 8), nj = 2: pass 2 reads columns 0, 257 and 281 of every group.  WALKED,
    and DECLINED with one key whose time goes back, so k_part2_hist and k_part2 read the coarse table with more than
    one column per group and the tiled walker delivers the push."""
    n = 2_300_000
    p = plan(65_700, n)
    assert (p["ns1"], p["nc1"], p["nsb"], p["tsb"], p["ts2"], p["nj"]) == (2_247, 281, 2, 1_128, 2_056, 2)
    rng = np.random.default_rng(77)
    keys = scattered_ids(rng, 2_000, bound=65_699, avoid=[65_600])
    keys[-1] = 65_699
    b = ordinary(rng, keys, n, T0, 0)
    seen = spy_routes(monkeypatch)
    if route == DECLINED:
        go_back(b, T0, key=65_600)
    parity(query(), [b], [route], min_matches=100_000)
    if route == DECLINED:
        assert "part_hist2" in seen[0] and "part_key" in seen[0] and "walk_count" in seen[0]


# ---- 5. the key bound grows between pushes

def test_key_bound_grows_between_pushes():
    """Three pushes of 20,000 rows on one handle (seg1 = 1024, ns1 = 20 or 21 with the carry, nc1 = 3, tsb = 24,
    nsb = 1, ts2 = 24, nj = 1): key bound 65,537 in push 1 (ng = 257, lbs = 3, nsg = 33: the group table has
    257 * 3 + 1 entries), 140,001 from push 2 on (ng = 547 > 512, lbs = 4, nsg = 35: 547 * 3 + 1 entries, the
    supergroup table 35 columns of ns1) -- both tables and the key bases (kb + 1 entries) grow on one handle, and
    push 2 walks carried rows of push 1.  Route: WALKED on every push."""
    rng = np.random.default_rng(61)
    n = 20_000
    keys = scattered_ids(rng, 1_200, bound=65_536)
    keys[-1] = 65_536
    more = np.concatenate([keys, scattered_ids(rng, 300, bound=140_000), [140_000]])
    p1, p2 = plan(65_537, n), plan(140_001, n + 3_000)
    assert (p1["ng"], p1["lbs"], p1["nc1"], p2["ng"], p2["lbs"], p2["nc1"]) == (257, 3, 3, 547, 4, 3)
    batches = [ordinary(rng, keys, n, T0, 0), ordinary(rng, more, n, T0 + 500, n),
               ordinary(rng, more, n, T0 + 1000, 2 * n)]
    want, per = parity(query(), batches, [WALKED] * 3, min_matches=10_000)
    assert (want.vals[per[0]:per[0] + per[1], 0] < n).any()   # push 2 completes partials of push 1


# ---- 6. k_gw_count: 16 bytes per lane between a scalar head and tail, key bases from the block's own scan

FALL = np.array([39.9, 39.8, 39.7, 39.95], np.float32)   # three falling candidates outgrow a ring of two; then a spike


@pytest.mark.parametrize("shift", [1, 6, 11, 16])
def test_gw_count_alignment(shift, monkeypatch):
    """k_gw_count's head / body / tail split (the group's range [lo, hi) of glk: bytes up to the next multiple of 16
    one per lane, whole 16-byte words, the rest one per lane) and its key bases.  Group 0 holds `shift` rows (1..16) in
    front, so the groups behind start at every offset: groups 1..16 hold 17 rows each (lo = shift + 17 i: all sixteen
    residues modulo 16, each with a head of 0..15 bytes, zero or one word and a tail), group 17 none, group 18 one row,
    19 fifteen, 20 sixteen, group 21 4,097 rows all of one key (in-group key 255: 4,096 of the block's exclusive sum sit
    on one lane), groups 22..272 none, and the last group (273, partial: key bound 70,001 = 273 * 256 + 113) holds four
    rows of its last key 70,000, whose base is followed by the end sentinel kbase[K].  Prices rise with every row, so a
    pending list never holds two -- but for key 70,000 and key 1,283 of group 5 (three falling prices, then a spike):
    with SG_DEBUG_GW_CAP=2 both outgrow the ring and k_gw_redo gathers their rows between kbase[k] and kbase[k + 1].
    About 4,700 rows: seg1 = 1024, ns1 = 5, W = 8, nc1 = 1, tsb = 8, nsb = 1, ts2 = 8, nj = 1.  Route: redone(2)."""
    monkeypatch.setenv("SG_DEBUG_GW_CAP", "2")
    rng = np.random.default_rng(90 + shift)
    rows = [rng.choice(256, shift, replace=True)]                                  # group 0
    for g in range(1, 17):
        lanes = rng.choice(256, 17, replace=True)
        if g == 5:
            lanes[:4] = 3                                                          # key 1,283: four rows
            lanes[4:][lanes[4:] == 3] = 4
        rows.append((g << 8) + lanes)
    rows.append((18 << 8) + np.array([200]))
    rows.append((19 << 8) + rng.choice(256, 15, replace=True))
    rows.append((20 << 8) + rng.choice(256, 16, replace=True))
    rows.append(np.full(4_097, (21 << 8) + 255))
    rows.append(np.full(4, 70_000))
    key = np.concatenate(rows)
    rng.shuffle(key)
    n = len(key)
    assert n == shift + 16 * 17 + 1 + 15 + 16 + 4_097 + 4
    counts = np.bincount(key >> 8, minlength=274)
    assert counts[:22].tolist() == [shift] + [17] * 16 + [0, 1, 15, 16, 4_097] and counts[22:273].sum() == 0
    lo = np.cumsum(counts) - counts
    assert sorted(lo[1:17] % 16) == list(range(16))
    p = plan(70_001, n)
    assert (p["ns1"], p["nc1"], p["nsb"], p["nj"]) == (5, 1, 1, 1)
    price = (np.float32(20.5) + np.arange(n, dtype=np.float32) * np.float32(19.0 / n)).astype(np.float32)
    for k in (70_000, (5 << 8) + 3):
        at = np.nonzero(key == k)[0]
        assert len(at) == 4
        price[at] = FALL
    b = stock(times(n, 40), key, price)
    want, _ = parity(query(), [b], [redone(2)], min_matches=1_000)
    for k in (70_000, (5 << 8) + 3):   # the spike delivers the three partials of the run, oldest first
        assert int((want.key == k).sum()) == 3
