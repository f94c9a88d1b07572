"""The device key dictionary (siddhi_amd/csrc/keydict.hip) through the node pipeline at the keys that are hard for it:
probe chains that wrap the table, the sentinel raw value INT64_MIN, chunks of duplicates racing on one slot, and table
rebuilds -- on one GPU (gpu_loop), through the shard exchange (G shards on device 0) and on the range-routing path;
the non-growth cases also through the host dictionary (router.cpp), against the same expectation.

Every expectation comes from keydict_cases.py: a row-at-a-time Python dict gives the ids, the oracle engine the matches
(test_keydict_cases.py guards the cases on the CPU).  Growth cases run with SG_DEBUG_KD_CAP=1024 (a test hook: the
initial capacity) and every case asserts, through sg_node_key_dict_stats, the capacity and the number of rebuilds of
every shard's table: no test passes without having taken the path it names."""
import dataclasses
import functools

import numpy as np
import pytest

import keydict_cases as KC
import node_range_cases as NC
from parity_util import assert_same, context
from siddhi_amd.runtime import Outputs
from test_node import node_outputs
from test_node_ranges import open_node, push as range_push

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

SG_EINVAL = -1
HOST, DEVICE = 1, 2


def run_case(c: KC.Case, gpus: int, key_dict: int):
    """The case through one node: (delivered Outputs per stream, key-dictionary stats per shard or None on the host
    dictionary, shard_rows after the last push).  node.keys() is checked after every push."""
    from siddhi_amd import _native as N
    nfa = __import__("siddhi_amd.lowering", fromlist=["lower"]).lower(context(KC.QUERY))
    node = N.Node(N.build_desc(nfa), n_gpus=gpus, devices=[0] * gpus, threads=4, chunk_rows=c.chunk)
    outs = []
    try:
        node.set_key_dict(key_dict)
        for lo, hi in KC.pieces(c):
            if lo == c.reset_at:
                node.reset()
            if lo == 0 or lo == c.reset_at:
                base = lo
                outs.append([])
            b = KC.batch(c, lo, hi, base)
            raw = np.ascontiguousarray(c.raw[lo:hi], np.int64)
            keep = [raw, b.ts, b.stream] + b.cols
            nb = N.make_node_batch(b.n, b.base_index, b.ts.ctypes.data, b.stream.ctypes.data, raw.ctypes.data,
                                   [x.ctypes.data for x in b.cols], [0, 0, 0], keep)
            sink = N.ColumnSink(nfa, 2 * b.n + 16, pinned=False)
            outs[-1].append(node_outputs(nfa, sink, node.push(nb, sink.struct, sink.cap)))
            assert node.keys() == KC.distinct_after(c, hi), (lo, hi)
        if key_dict == DEVICE:
            stats = [node.key_dict_stats(s) for s in range(gpus)]
            for bad in (-1, gpus):
                with pytest.raises(N.SgError) as ei:
                    node.key_dict_stats(bad)
                assert ei.value.code == SG_EINVAL
        else:
            stats = None
            with pytest.raises(N.SgError) as ei:      # no device dictionary to report on
                node.key_dict_stats(0)
            assert ei.value.code == SG_EINVAL
        shard_rows = node.stats()["shard_rows"][:gpus]
    finally:
        node.close()
    return [Outputs(*[np.concatenate([getattr(o, f) for o in s]) for f in KC.FIELDS]) for s in outs], stats, shard_rows


def check_case(name, gpus, key_dict=DEVICE, scale=1):
    c = KC.case(name, scale)
    got, stats, shard_rows = run_case(c, gpus, key_dict)
    ids = KC.ref_ids(c)
    spans = KC.streams(c)
    assert len(got) == len(spans)
    for g, w, (lo, hi) in zip(got, KC.want(name, scale), spans):
        assert_same(g, w)
        # without the oracle: a match's key is the reference id of the raw key of its trigger row
        assert np.array_equal(g.key, ids[lo + g.trigger.astype(np.int64)])
    if stats is not None:
        # the shard of every row is the product's hash of its raw key (the last stream: a reset clears the counts; the
        # exchange drops clock-only rows, one GPU passes them on)
        lo, hi = spans[-1]
        keyed = ~c.is_clock()[lo:hi] if gpus > 1 else np.ones(hi - lo, bool)
        assert shard_rows == np.bincount(KC.shard_of(c.raw[lo:hi], gpus)[keyed], minlength=gpus).tolist()
        _, want_stats = KC.model(c, gpus)
        assert stats == want_stats
        grew = [t["rebuilds"] for t in stats]
        if name in KC.GROWTH:
            assert min(grew) >= 1 and all(t["cap"] == KC.SMALL_CAP << (2 * t["rebuilds"]) for t in stats)
        else:
            assert max(grew) == 0 and all(t["cap"] == KC.KD_MIN_CAP for t in stats)
    return stats


@pytest.mark.parametrize("route", ["g1", "g2", "g3", "host1", "host2"])
@pytest.mark.parametrize("name", list(KC.PLAIN))
def test_plain_cases(name, route, monkeypatch):
    """chains, the sentinel, duplicates, chunk edges, pushes and clock-only rows in the production table (4M slots, no
    rebuild): gpu_loop, the exchange over 2 and 3 shards, and the host dictionary (one and two shards) against the
    same expectation"""
    monkeypatch.delenv("SG_DEBUG_KD_CAP", raising=False)
    check_case(name, int(route[-1]), HOST if route.startswith("host") else DEVICE)


@pytest.mark.parametrize("gpus", [1, 2])
@pytest.mark.parametrize("name", list(KC.GROWTH))
def test_growth_cases(name, gpus, monkeypatch):
    """from 1024 slots: the case is sized per shard, so every shard's table rebuilds on either route"""
    monkeypatch.setenv("SG_DEBUG_KD_CAP", str(KC.SMALL_CAP))
    stats = check_case(name, gpus, scale=gpus)
    if gpus == 1:
        want = {"grow_twice": (2, 16384)}.get(name, (1, 4096))
        assert (stats[0]["rebuilds"], stats[0]["cap"]) == want


@pytest.mark.parametrize("value", ["1000", "512", "8388608", "4096x", ""])
def test_capacity_hook_refuses_other_values(value, monkeypatch):
    """not a power of two, under 1024, over the production capacity, not a number: the push fails with SG_EINVAL and
    says why; the hook is never ignored"""
    from siddhi_amd._native import SgError
    monkeypatch.setenv("SG_DEBUG_KD_CAP", value)
    with pytest.raises(SgError) as ei:
        run_case(KC.case("sentinel_first"), 1, DEVICE)
    assert ei.value.code == SG_EINVAL and "SG_DEBUG_KD_CAP" in str(ei.value)


# ------------------------------------------------------------------------------------------- range partitions
@functools.lru_cache(maxsize=None)
def _sentinel_label() -> NC.Prepared:
    """the three-range case of test_node_ranges.py with INT64_MIN as the raw key of label 'low'"""
    c = NC.case("core")
    return NC.Prepared(dataclasses.replace(c, raw={**c.raw, "low": KC.I64_MIN}, apart=()))


@functools.lru_cache(maxsize=None)
def _many_value_keys() -> NC.Prepared:
    """S keyed by 880 values, T by 24 ranges: 900 keys in one chunk.  Four labels are strings of their own; twenty are
    the strings of values 37, 74, ..., so those instances see both streams and their ids -- spread over the whole
    first-seen order -- show in the matches."""
    labels = ["a", "b", "c", "d"] + [str(37 * i) for i in range(1, 21)]
    text = ("define stream S (k int); define stream T (v int); partition with (k of S, " +
            " or ".join(f"v>{50 * i} as '{lab}'" for i, lab in enumerate(labels)) +
            " of T) begin @info(name='q') from every e1=S -> e2=T[v>e1.k] select e1.k as k, e2.v as v insert into M; end;")
    rng = np.random.default_rng(3)
    rows, t = [], 0
    for again in range(2):      # (T rows in the second round only: the labels shared with values keep early ids)
        for k in rng.permutation(880):
            rows.append((0, t, [int(k)]))
            t += 2
            if again and k % 3 == 0:
                rows.append((1, t - 1, [int(rng.integers(0, 2000))]))
    raw = {name: 5000 + i for i, name in enumerate(labels[:4] + [str(k) for k in range(880)])}
    return NC.Prepared(NC.Case(text, rows, raw, value_key={0: 0}, cap_per_row=30))


def run_ranges(p: NC.Prepared, gpus):
    node = open_node(p, gpus)
    try:
        got = range_push(node, p, 0, len(p.case.rows))
        keys = node.keys()
        stats = [node.key_dict_stats(s) for s in range(gpus)]
    finally:
        node.close()
    assert_same(got, p.want)
    assert len(p.want) > 0 and keys == len(p.routed.keys) == sum(t["n_keys"] for t in stats)
    return stats


@pytest.mark.parametrize("gpus", [1, 2])
def test_range_label_with_the_sentinel_raw(gpus, monkeypatch):
    monkeypatch.delenv("SG_DEBUG_KD_CAP", raising=False)
    stats = run_ranges(_sentinel_label(), gpus)
    assert all(t["rebuilds"] == 0 and t["cap"] in (0, KC.KD_MIN_CAP) for t in stats)
    assert stats[int(KC.shard_of(np.array([KC.I64_MIN]), gpus)[0])]["cap"] == KC.KD_MIN_CAP


def test_range_labels_and_value_keys_cross_the_limit(monkeypatch):
    """one chunk of 884 new keys (labels and value keys) in a 1024-slot table: past 512 + 256, under 2048"""
    monkeypatch.setenv("SG_DEBUG_KD_CAP", str(KC.SMALL_CAP))
    p = _many_value_keys()
    assert len(p.routed.keys) == 884 and len(set(p.want.key.tolist())) == 20 and p.want.key.max() > 800
    assert run_ranges(p, 1) == [dict(cap=4096, n_keys=884, rebuilds=1, probes=2)]
