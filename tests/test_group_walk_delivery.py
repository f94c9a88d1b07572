"""How a group-walked push delivers (csrc/gwalk.h): trigger words tagged with a per-push epoch instead of a zero fill
per push (gw_tagged_words, gw_trig_word; a word of another epoch is no trigger to k_gtile_count and k_gscan_project),
and the tile counts, tile bases and tile projection that turn them into records.

Every case is small, every handle sees a key id >= 65,536 (so the wide partition and the group walker run), every case
is compared row for row with the oracle and asserts the route of every push (test_group_walk_edges.parity), and no
push may raise SgError: the group walker's internal checks (its guards, the match count of the scan against the
walkers') never fire on a correct build (`delivered` turns an SgError into a failure that says so)."""
import numpy as np
import pytest

from siddhi_amd._native import SgError
from siddhi_amd.runtime import Batch
from test_group_walk import query
from test_group_walk_edges import (DECLINED, SELECTS, T0, WALKED, ordinary, parity, prices, redone, round_robin,
                                   scattered_ids, stock, times)

pytestmark = pytest.mark.gpu


def delivered(q, batches, routes=None, **kw):
    """parity with the oracle and the route of every push (default WALKED); no push raises SgError"""
    try:
        return parity(q, batches, routes or [WALKED] * len(batches), **kw)
    except SgError as e:
        pytest.fail(f"a push raised SgError (an internal check of the group walker fired): {e}")


def key_set(rng, count=1_500, avoid=()):
    keys = scattered_ids(rng, count, avoid=list(avoid) + [70_000])
    keys[-1] = 70_000   # the sparse id past 65,535 that every handle sees
    return keys


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2_048, 2_049, 70_000])
def test_tile_shapes(n):
    """a push of n rows behind a 3,000-row push that leaves partials on every key: one row, one row under / exactly /
    one row over a 256-row tile, a whole workgroup of k_gtile_count (eight tiles) and one row more, and 274 tiles (the
    scan over the tile counts takes more than one block).  The one-row push completes carried partials of its key, so
    it delivers."""
    rng = np.random.default_rng(3)
    keys = key_set(rng)
    b1 = ordinary(rng, keys, 3_000, T0, 0)
    b2 = ordinary(rng, keys, n, T0 + 75, 3_000)
    b2.cols[2][0] = np.float32(39.75)   # above every carried price of its key
    _, per = delivered(query(), [b1, b2])
    assert per[1] >= 1
    if n >= 255:
        assert per[1] > n // 4


def test_gap_in_the_middle():
    """3,000 rows with triggers, 57,000 rows of globally falling price (candidates that complete nothing under `>`:
    222 tiles whose count is zero and whose base is the same), then 10,000 rows with triggers that also complete what
    the gap left pending."""
    rng = np.random.default_rng(5)
    n, lo, hi = 70_000, 3_000, 60_000
    keys = key_set(rng, 2_000)
    price = prices(rng, n, 30.0, 39.0)
    price[lo:hi] = np.float32(38.0) - np.arange(hi - lo, dtype=np.float32) * np.float32(17.0 / (hi - lo))
    price[hi:] = prices(rng, n - hi, 25.0, 39.5)
    b = stock(times(n, 20), round_robin(keys, n), price)
    want, _ = delivered(query(), [b], min_matches=1000)
    assert not ((want.trigger >= lo + len(keys)) & (want.trigger < hi)).any()   # (the gap's first row per key may trigger)
    assert (want.trigger < lo).any() and (want.trigger >= hi).any()


def test_multi_round_tile():
    """one key with a rising run of 300 candidates under `<` (nothing completes), then a row below all of them: one
    trigger of 300 matches, more than GW_PROJ_S (256), so its tile stores in two rounds and the trigger straddles them.
    The key's list outgrows the ring: redone()."""
    rng = np.random.default_rng(7)
    n, deep = 20_000, 66_200
    keys = key_set(rng, 2_000, avoid=[deep])
    key = round_robin(keys, n).astype(np.int64)
    price = prices(rng, n)
    run = 2_000 + 20 * np.arange(300)
    key[run], price[run] = deep, np.float32(21.0) + np.arange(300, dtype=np.float32) * np.float32(0.05)
    key[9_000], price[9_000] = deep, np.float32(20.5)
    want, _ = delivered(query("price < e1.price"), [stock(times(n, 40), key, price)], [redone()], min_matches=1000)
    assert int((want.trigger == 9_000).sum()) == 300


def test_no_matches():
    """a push in which every price is the same (`>` completes no tie: no match, the projection is skipped and the
    epoch still advances), then a push with matches, some of them completing what the first left pending"""
    rng = np.random.default_rng(9)
    keys = key_set(rng)
    b1 = ordinary(rng, keys, 8_000, T0, 0)
    b1.cols[2][:] = np.float32(25.0)
    b2 = ordinary(rng, keys, 8_000, T0 + 200, 8_000)
    want, per = delivered(query(), [b1, b2], min_matches=1000)
    assert per[0] == 0 and (want.vals[:, 0] < 8_000).any()


def test_stale_words(monkeypatch):
    """ten carried pushes of changing size on one handle with the epochs wrapping after three
    (SG_DEBUG_GW_EPOCHS=3): pushes 4, 7 and 10 start again at epoch 1 over words the pushes before them tagged 1, 2
    and 3, and a shorter push leaves a longer one's words behind it.  Every push's output is the oracle's, so a row
    that triggered in one push triggers in the next only where the oracle says so; the trigger positions do differ."""
    monkeypatch.setenv("SG_DEBUG_GW_EPOCHS", "3")
    rng = np.random.default_rng(13)
    keys = key_set(rng)
    sizes = [6_000, 5_000, 6_500, 4_000, 6_500, 3_000, 6_000, 6_000, 2_000, 6_500]
    batches, base = [], 0
    for i, m in enumerate(sizes):
        batches.append(ordinary(rng, keys, m, T0 + 200 * i, base))
        base += m
    want, per = delivered(query(), batches, min_matches=10_000)
    assert all(p > 500 for p in per)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    pos = [set((np.unique(want.trigger[(want.trigger >= starts[i]) & (want.trigger < starts[i + 1])]) - starts[i]).tolist())
           for i in range(len(sizes))]
    for i in range(len(sizes) - 1):
        gone = [p for p in pos[i] - pos[i + 1] if p < sizes[i + 1]]
        assert len(gone) > 100, (i, len(gone))   # positions that triggered in push i and must not in push i + 1


def test_grow():
    """5,000 rows, then 60,000 on the same handle (the trigger-word workspace is allocated anew and the words past the
    old high-water mark are cleared), then 5,000 again (under the 60,000-row push's words)"""
    rng = np.random.default_rng(17)
    keys = key_set(rng)
    b1 = ordinary(rng, keys, 5_000, T0, 0)
    b2 = ordinary(rng, keys, 60_000, T0 + 125, 5_000)
    b3 = ordinary(rng, keys, 5_000, T0 + 1_625, 65_000)
    _, per = delivered(query(), [b1, b2, b3], min_matches=10_000)
    assert all(p > 1000 for p in per)


def test_after_decline():
    """the handle's first push is declined with GW_ORDER after k_gwalk has written trigger words (key 66,010: rows at
    +100 ms, +50 ms -- its time goes back -- and +200 ms, which completes both); those words carry an epoch the next
    push does not use.  Pushes 2 and 3 are WALKED."""
    rng = np.random.default_rng(23)
    n = 20_000
    keys = key_set(rng, avoid=[66_010])
    b1 = ordinary(rng, keys, n, T0, 0)
    b2 = ordinary(rng, keys, n, T0 + 500, n)
    b3 = ordinary(rng, keys, n, T0 + 1000, 2 * n)
    for row, dt, p in [(4_000, 100, 30), (4_001, 50, 25), (8_000, 200, 50)]:
        b1.key[row] = b1.cols[1][row] = 66_010
        b1.ts[row] = T0 + dt
        b1.cols[2][row] = np.float32(p)
    want, per = delivered(query(), [b1, b2, b3], [DECLINED, WALKED, WALKED], min_matches=10_000)
    assert all(p > 1000 for p in per)
    assert want.vals[want.key == 66_010, :2].tolist()[:2] == [[4_000, 8_000], [4_001, 8_000]]


def test_redo(monkeypatch):
    """a redone key under epoch 2 and under epoch 1 after a wrap (SG_DEBUG_GW_EPOCHS=2, SG_DEBUG_GW_CAP=2): the
    background's prices rise with every row (each row completes the one before it: no list holds two), and in pushes 2
    and 3 one key gets a falling run of five and then a price above them, which outgrows the ring of two; k_gw_redo
    writes the key's trigger words again under the epoch of the first walk.  Routes: WALKED, redone(), redone()."""
    monkeypatch.setenv("SG_DEBUG_GW_CAP", "2")
    monkeypatch.setenv("SG_DEBUG_GW_EPOCHS", "2")
    rng = np.random.default_rng(29)
    n, deep = 8_000, 66_300
    keys = key_set(rng, avoid=[deep])
    batches = []
    for i in range(3):
        b = ordinary(rng, keys, n, T0 + 200 * i, i * n)
        b.cols[2][:] = np.float32(20.5) + (i * n + np.arange(n, dtype=np.float32)) * np.float32(17.0 / (3 * n))
        if i:
            run = 1_000 + 37 * i + 50 * np.arange(6)
            b.key[run] = b.cols[1][run] = deep
            b.cols[2][run[:-1]] = np.float32(39.0) - np.arange(5, dtype=np.float32) * np.float32(0.5)
            b.cols[2][run[-1]] = np.float32(39.9)
        batches.append(b)
    want, _ = delivered(query(), batches, [WALKED, redone(), redone()], min_matches=10_000)
    for i in (1, 2):
        # (push 3 also finds push 2's 39.9 carried; a tie completes nothing under `>`)
        assert int((want.trigger == i * n + 1_000 + 37 * i + 250).sum()) == 5


def test_odd_select():
    """three select columns: the record stride is 8 mod 16, so a tile that ends on an odd slot takes the projection's
    8-byte tail store and one that starts on an odd slot its 8-byte branch; two pushes polled once, so the second
    writes behind the first's records"""
    rng = np.random.default_rng(31)
    keys = key_set(rng)
    b1 = ordinary(rng, keys, 9_001, T0, 0)
    b2 = ordinary(rng, keys, 9_000, T0 + 225, 9_001)
    delivered(query(select=SELECTS[3]), [b1, b2], min_matches=1000, fetch_after=[1])


def test_index_column():
    """batches that carry an index column (a rank's share of a stream: the trigger is index[b], not base + b)"""
    rng = np.random.default_rng(37)
    keys = key_set(rng)
    batches = []
    for i in range(2):
        b = ordinary(rng, keys, 9_000, T0 + 225 * i, 9_000 * i)
        ix = np.uint64(7) + np.uint64(3) * (np.uint64(9_000 * i) + np.arange(9_000, dtype=np.uint64))
        batches.append(Batch(b.n, b.base_index, b.ts, b.stream, b.key, b.cols, b.nulls, index=ix))
    want, _ = delivered(query(), batches, min_matches=1000)
    assert (want.trigger % 3 == 1).all() and int(want.trigger.max()) > 3 * 9_000
