"""GPU parity for the two key-partition paths of the closed-form walker (siddhi_amd/csrc/keypart.h): the
LDS-staged counting partition (one pass for key_bound <= 256, two passes up to 65536) and the rocPRIM radix
sort (sg_options.partition_sort = 1, and every key_bound above 65536).  Both must hand the walkers each key's
rows in arrival order -- the routing of PartitionStreamReceiver (C/partition/PartitionStreamReceiver.java:80-281)
-- so the match sequences are identical to the oracle's, bit for bit, across digit boundaries (256/257 keys,
ragged last groups), skewed keys, sub-tile edges and multi-push carry."""
import numpy as np
import pytest

from oracle import OracleEngine
from parity_util import assert_same, dense_first_seen, run_engine, synth_batch
from siddhi_amd import synth
from siddhi_amd.runtime import Batch

pytestmark = pytest.mark.gpu

APP = synth.QUERIES["C2"]


def _engine(sort):
    from siddhi_amd._native import GpuEngine
    return lambda ctx: GpuEngine(ctx, partition_sort=sort)


def _batch(n, keys, seed, skew=False, rate=50):
    rng = np.random.default_rng(seed)
    if skew:   # a few hot keys and a long tail (uneven digit runs, empty keys)
        key = np.minimum(rng.zipf(1.3, size=n) - 1, keys - 1).astype(np.int32)
    else:
        key = rng.integers(0, keys, size=n).astype(np.int32)
    ts = 1_700_000_000_000 + np.arange(n, dtype=np.int64) // rate
    price = rng.integers(0, 1000, size=n).astype(np.float32) / 10
    ids = np.arange(n, dtype=np.int64)
    return Batch(n, 0, ts, np.zeros(n, np.int32), dense_first_seen(key), [ids, key.copy(), price], [None] * 3)


@pytest.mark.parametrize("n,keys,skew", [
    (5_000, 1, False), (20_000, 7, False), (50_000, 256, False), (50_000, 257, False), (60_000, 300, True),
    (70_001, 5_000, False), (100_000, 16_384, True), (90_000, 65_536, False), (80_000, 70_000, False)])
def test_partition_paths_match_oracle(n, keys, skew):
    b = _batch(n, keys, seed=keys + n, skew=skew)
    want = run_engine(OracleEngine, APP, [b])
    for sort in (0, 1):
        got = run_engine(_engine(sort), APP, [b])
        assert_same(got, want)


def test_partition_multi_push_carry():
    b = _batch(120_000, 3_000, seed=5)
    parts, lo = [], 0
    for hi in (17_000, 50_001, 90_000, b.n):
        parts.append(Batch(hi - lo, lo, b.ts[lo:hi], b.stream[lo:hi], b.key[lo:hi], [c[lo:hi] for c in b.cols],
                           [None] * 3))
        lo = hi
    want = run_engine(OracleEngine, APP, parts)
    assert_same(run_engine(_engine(0), APP, parts), want)


def test_partition_large_batch_against_radix_sort():
    """Many pass-1 segments and pass-2 segments spanning several sub-tiles (4M rows): both paths agree."""
    b = synth_batch("C2", 0, 4_000_000, keys=10_000, rate=1_000)
    b.key = dense_first_seen(b.key)
    a = run_engine(_engine(0), APP, [b])
    r = run_engine(_engine(1), APP, [b])
    assert len(a) > 100_000
    assert_same(a, r)
