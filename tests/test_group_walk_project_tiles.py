"""The group walker's delivery side with a trigger per thread (csrc/gw_proj.h: k_gtile_count, k_gscan_project<RPT>;
csrc/gwalk.h: gw_project): a workgroup takes a tile of R = 256 * RPT arrival rows, reads their trigger words 16 bytes at a time,
compacts the tile's triggers into a list in LDS and hands list entry i to thread i mod 256, which reads the header and
the two entries behind it before it uses either.  Every case runs for RPT 1, 2 and 4 (SG_DEBUG_GW_PROJ_RPT), row for
row against the oracle, on pushes of 10^2 .. 10^4 rows with a key id past 65,535 (the wide partition, as
test_group_walk_edges), and asserts from the kernels the handle timed that "gw_project" delivered the matches.

Where the new code can go wrong: the tile's ragged end (n = R - 1, R, R + 1, 2R + 1: the 16-byte load that would
cross n, the scalar tail), a list at its bound (every row of a tile triggers), a tile without a trigger between two
with some, a trigger of exactly 1, 2 and 3 matches (the two entries read with the header, then the loop) and of more
than GW_PROJ_S at a tile's first and last row, the trigger that ends the match area, odd and even record strides at a
zero and a non-zero (with an odd stride: unaligned) out_base, the index column, and stale words of another epoch."""
import functools

import numpy as np
import pytest

import test_group_walk_edges as edges
from oracle import OracleEngine
from parity_util import run_engine
from siddhi_amd.runtime import Batch
from test_group_walk import pieces, query
from test_group_walk_edges import T0, WALKED, parity, prices, redone, round_robin, scattered_ids, stock, times

pytestmark = pytest.mark.gpu

TOP = 70_000   # the highest key id of every case: the key bound is 70,001, the wide partition runs
SELECTS = {1: "e1.id as a",
           4: "e1.id as a, e2.id as b, e1.price as c, e2.price as d",
           5: "e1.id as a, e2.id as b, e1.price as c, e2.price as d, e1.id as e"}


@pytest.fixture(params=[1, 2, 4], ids=lambda r: f"rpt{r}")
def R(request, monkeypatch):
    """selects k_gscan_project<RPT>; the rows of a tile"""
    monkeypatch.setenv("SG_DEBUG_GW_PROJ_RPT", str(request.param))
    return 256 * request.param


@pytest.fixture
def seen(monkeypatch):
    """the timed kernel names of every push parity() drives, in order"""
    log = []
    real = edges.check_route

    def record(route, names, spilled, emitted, where):
        log.append(list(names))
        real(route, names, spilled, emitted, where)

    monkeypatch.setattr(edges, "check_route", record)
    return log


def key_ids(rng, count, avoid=()):
    """`count` scattered ids, TOP among them"""
    ids = scattered_ids(rng, count - 1, bound=TOP, avoid=avoid)
    return np.concatenate([ids, [TOP]])


def ordinary(rng, ids, n, start=T0, base=0):
    return stock(times(n, 40, start), round_robin(ids, n), prices(rng, n, 21, 38), base=base)


# ---- tile edges

@pytest.mark.parametrize("rows", ["R-1", "R", "R+1", "2R+1"])
def test_tile_edges(R, rows, seen):
    """n one row short of a tile, exactly one, one more and one more than two: the last tile's rows past n read as no
    trigger, the pair of words that would cross n is read as one word, and k_gtile_count's last tile is partial.  The
    batch's last row triggers (price 1000 completes what its key holds)."""
    n = {"R-1": R - 1, "R": R, "R+1": R + 1, "2R+1": 2 * R + 1}[rows]
    rng = np.random.default_rng(3)
    b = ordinary(rng, key_ids(rng, 20), n)
    b.cols[2][-1] = np.float32(1000)
    want, _ = parity(query(), [b], [WALKED], min_matches=n // 8)
    assert "gw_project" in seen[0] and "gw_tiles" in seen[0]
    assert int((want.trigger == n - 1).sum()) >= 1


# ---- a list at its bound

def test_dense_tile(R, seen):
    """64 keys in turn with prices rising row by row: every row but each key's first completes exactly its key's row
    before it, so every row of the second and third tile is a trigger and the LDS list holds R entries"""
    rng = np.random.default_rng(5)
    n = 3 * R
    b = stock(times(n, 40), round_robin(key_ids(rng, 64), n),
              np.float32(21) + np.arange(n, dtype=np.float32) * np.float32(0.005))
    want, _ = parity(query(), [b], [WALKED], min_matches=n - 64)
    assert len(want) == n - 64 and "gw_project" in seen[0]
    assert np.array_equal(np.unique(want.trigger), np.arange(64, n))


# ---- sparse tiles

def test_sparse_tiles(R, seen):
    """a tile without a trigger (its rows pass neither filter: price 10) between two tiles with some; then a push
    without a match (nothing is projected) and a third that delivers again"""
    rng = np.random.default_rng(7)
    ids = key_ids(rng, 50)
    b1 = ordinary(rng, ids, 3 * R + 7)
    b1.cols[2][R:2 * R] = np.float32(10)
    b2 = ordinary(rng, ids, R + 3, T0 + 100, b1.n)
    b2.cols[2][:] = np.float32(10)
    b3 = ordinary(rng, ids, 2 * R + 9, T0 + 200, b1.n + b2.n)
    want, per = parity(query(), [b1, b2, b3], [WALKED] * 3, min_matches=R)
    assert per[0] > R // 4 and per[1] == 0 and per[2] > R // 4
    assert "gw_project" in seen[0] and "gw_project" not in seen[1] and "gw_project" in seen[2]
    first = want.trigger[:per[0]]
    assert (first < R).any() and (first >= 2 * R).any() and not ((first >= R) & (first < 2 * R)).any()


# ---- match counts at the first and the last row of a tile

COUNTS = [1, 2, 3, 300]


def counts_batch(R):
    """six tiles of background (300 keys in turn) and eight keys whose only trigger completes a falling run of 1, 2, 3
    and 300 candidates: at the first row of tiles 1..4 and at the last row of tiles 1..4.  The run's rows are the free
    rows closest below the trigger."""
    rng = np.random.default_rng(9)
    n = 6 * R
    special = [66_500 + j for j in range(8)]
    b = ordinary(rng, key_ids(rng, 300, avoid=special), n)
    spikes = [R * (j + 1) for j in range(4)] + [R * (j + 2) - 1 for j in range(4)]
    used = set(spikes)
    for k, c, at in zip(special, COUNTS + COUNTS, spikes):
        run = []
        r = at - 1
        while len(run) < c:
            if r not in used:
                run.append(r)
                used.add(r)
            r -= 1
        assert r >= 0
        run = np.asarray(run[::-1])
        for rows, p in ((run, np.float32(39.5) - np.arange(c, dtype=np.float32) * np.float32(0.05)),
                        ([at], np.float32(39.9))):
            b.key[rows] = b.cols[1][rows] = k
            b.cols[2][rows] = p
    return b, list(zip(COUNTS + COUNTS, spikes))


def test_match_counts(R, seen):
    """triggers of exactly 1 and 2 matches (the entries read with the header cover them), 3 (the first that loops over
    a further entry) and 300 (more than GW_PROJ_S: the trigger straddles staging rounds), each at the first and at the
    last row of a tile.  The two 300-deep runs outgrow the ring: redone(2)."""
    b, placed = counts_batch(R)
    want, _ = parity(query(), [b], [redone(2)], min_matches=600)
    assert "gw_project" in seen[0]
    for c, at in placed:
        assert at % R in (0, R - 1)
        assert int((want.trigger == at).sum()) == c, (c, at)


# ---- the end of the match area

@pytest.mark.parametrize("m", [1, 2, 3])
def test_end_of_match_area(R, m, seen):
    """the highest key's last row is the batch's last row and completes a falling run of m: its header and entries are
    the last used units of the match area, and with m == 1 the second entry read with the header lies behind them"""
    rng = np.random.default_rng(11)
    n = 2 * R + 5
    b = ordinary(rng, scattered_ids(rng, 40, bound=TOP), n)
    rows = n - 1 - 3 * np.arange(m + 1)[::-1]
    b.key[rows] = b.cols[1][rows] = TOP
    b.cols[2][rows[:-1]] = np.float32(39.5) - np.arange(m, dtype=np.float32) * np.float32(0.25)
    b.cols[2][rows[-1]] = np.float32(39.9)
    assert b.key.max() == TOP and b.key[-1] == TOP
    want, _ = parity(query(), [b], [WALKED], min_matches=R // 4)
    assert "gw_project" in seen[0]
    assert int((want.trigger == n - 1).sum()) == m and (want.key[want.trigger == n - 1] == TOP).all()


# ---- strides and offsets

def stream_of(R):
    rng = np.random.default_rng(13)
    return ordinary(rng, key_ids(rng, 60), 4 * R + 11)


@functools.lru_cache(maxsize=None)
def odd_cut(R):
    """a cut of stream_of(R) after which the first push has delivered an odd number of matches"""
    b = stream_of(R)
    for cut in range(2 * R + 1, 2 * R + 40):
        if len(run_engine(OracleEngine, query(), pieces(b, [cut])[:1])) % 2 == 1:
            return cut
    raise AssertionError("no cut with an odd first push")


def two_pushes(R, nsel):
    return query(select=SELECTS[nsel]), pieces(stream_of(R), [odd_cut(R)])


@pytest.mark.parametrize("poll", ["between", "once"])
@pytest.mark.parametrize("nsel", [1, 4, 5])
def test_strides_and_offsets(R, nsel, poll, seen):
    """select lists of 1, 4 and 5 columns (record strides 40, 64 and 72: 8 mod 16, 0 mod 16, 8 mod 16) over two pushes
    polled after each (out_base 0 twice) and polled once (the second push writes behind an odd number of records: with
    an odd stride its first tile starts on an 8-byte boundary and stores through the 8-byte branch)"""
    q, batches = two_pushes(R, nsel)
    parity(q, batches, [WALKED, WALKED], min_matches=R, fetch_after=None if poll == "between" else [1])
    assert "gw_project" in seen[0] and "gw_project" in seen[1]


def test_index_column(R, seen):
    """batches that carry an index column: the trigger of a record is index[b] of the list entry's row"""
    rng = np.random.default_rng(17)
    ids = key_ids(rng, 60)
    batches = []
    for i in range(2):
        n = 2 * R + 3
        b = ordinary(rng, ids, n, T0 + 100 * i, n * i)
        ix = np.uint64(7) + np.uint64(3) * (np.uint64(n * i) + np.arange(n, dtype=np.uint64))
        batches.append(Batch(b.n, b.base_index, b.ts, b.stream, b.key, b.cols, b.nulls, index=ix))
    want, _ = parity(query(), batches, [WALKED, WALKED], min_matches=R)
    assert "gw_project" in seen[0] and "gw_project" in seen[1]
    assert (want.trigger % 3 == 1).all() and int(want.trigger.max()) > 3 * (2 * R + 3)


# ---- stale words

def test_stale_words(R, seen, monkeypatch):
    """three pushes with the epochs wrapping after two (SG_DEBUG_GW_EPOCHS=2): the second push reads, in every tile,
    the first push's words of epoch 1 beside its own of epoch 2 (and is shorter, so its last tile ends among them);
    the third starts again at epoch 1 after the clear of a wrap"""
    monkeypatch.setenv("SG_DEBUG_GW_EPOCHS", "2")
    rng = np.random.default_rng(19)
    ids = key_ids(rng, 60)
    sizes = [3 * R + 5, 2 * R + 1, 3 * R + 5]
    batches, base = [], 0
    for i, n in enumerate(sizes):
        batches.append(ordinary(rng, ids, n, T0 + 100 * i, base))
        base += n
    _, per = parity(query(), batches, [WALKED] * 3, min_matches=R)
    assert all(p > R // 4 for p in per)
    assert all("gw_project" in names for names in seen)
