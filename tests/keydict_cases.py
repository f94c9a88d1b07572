"""Cases for the device key dictionary (siddhi_amd/csrc/keydict.hip) through the node pipeline, shared by
test_keydict_gpu.py (GPU) and test_keydict_cases.py (CPU, which guards the cases themselves).  Pure numpy.

The reference is a row-at-a-time Python dict over the raw 64-bit keys: a key's id is the number of distinct keys seen
before its first row, in stream order across chunks and pushes, restarting after a reset (ref_ids).  Expected matches
are the oracle engine's over those dense ids.  The query passes every row (prices rise row by row, the whole stream
lies inside `within`), so a key with r rows emits r - 1 matches and every key has at least two rows.

Adversarial keys come from a Python restatement of the table's hash (kd_home: Fibonacci hashing, the top log2(cap) bits
of raw * M).  M is odd, so INV = M^-1 mod 2^64 exists and the keys INV * ((H << 42) + j), j = 0, 1, ..., all have home
slot H in a 4M-slot table and H >> (22 - c) in a table of 2^c slots: one probe chain, at every capacity.

model() restates, on the host, how many rebuilds each shard's table must make: a chunk that brings D new keys to a
table of n_keys keys fits for certain when n_keys + D < cap / 2 (every claim is admitted) and is rebuilt for certain
when n_keys + D > cap / 2 + (probing threads) (not every claim can be admitted, even with each thread's overshoot of
one).  Between the two the outcome depends on timing; model() refuses such a case (Ambiguous) and the CPU guard keeps
every case out of that band on every route it runs on."""
import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from siddhi_amd import synth
from siddhi_amd.router import mix64
from siddhi_amd.runtime import Batch, Outputs

QUERY = synth.QUERIES["C2"]      # every e1=S[price>20] -> e2=S[price>e1.price] within 1 sec, partitioned by symbol
FIELDS = ("trigger", "ts", "key", "group", "vals", "vnull")

M = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
INV = pow(M, -1, 1 << 64)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
KD_MIN_CAP = 1 << 22             # the production initial capacity
KD_BLOCK, KD_MAX_BLOCKS = 256, 1024
SMALL_CAP = 1024                 # SG_DEBUG_KD_CAP of the growth cases: claims are admitted below 512
LAST = KD_MIN_CAP - 1            # home slot of the wrap chains: the last slot of every capacity from 1024 to 4M
MID = (1 << 21) + 12345
NEIGHBOURS = (I64_MAX, 1, 0, -1, I64_MIN + 1)    # ordinary keys next to the sentinel, in descending raw order
RULES = ("ascending_raw", "slot_order", "last_occurrence", "per_chunk", "sentinel_fresh")


def s64(u: int) -> int:
    u &= MASK
    return u - (1 << 64) if u >> 63 else u


def kd_home(raw: int, cap: int) -> int:
    """keydict.hip's kd_home for a table of `cap` slots"""
    return (((int(raw) & MASK) * M) & MASK) >> (64 - (cap.bit_length() - 1))


def chain_keys(home: int, count: int, first: int = 0) -> List[int]:
    """`count` distinct raw keys whose home slot in a 4M-slot table is `home`"""
    return [s64(INV * ((home << 42) + j)) for j in range(first, first + count)]


def spread_keys(count: int, salt: int) -> List[int]:
    """benign keys (the suite's usual splitmix64 symbols)"""
    return [int(x) for x in synth.raw_symbols(np.arange(count, dtype=np.int64) + salt * 1_000_003)]


def probe_threads(cap: int, rows: int) -> int:
    """threads of one k_kd_probe launch over `rows` rows of a `cap`-slot table"""
    blocks = max(1, min(KD_MAX_BLOCKS, cap // (4 * KD_BLOCK)))
    return KD_BLOCK * min(blocks, max(1, -(-rows // KD_BLOCK)))


@dataclass
class Case:
    name: str
    raw: np.ndarray                      # int64 per row
    chunk: int                           # the node's chunk_rows
    cuts: Tuple[int, ...] = ()           # the rows are pushed in pieces cut here
    cap0: int = KD_MIN_CAP               # initial capacity (SMALL_CAP: the growth cases)
    reset_at: Optional[int] = None       # sg_node_reset before the push that starts at this cut
    clock: Optional[np.ndarray] = None   # bool per row: a clock-only row (stream -1)
    scale: int = 1                       # growth cases are built per shard count

    def is_clock(self) -> np.ndarray:
        return np.zeros(len(self.raw), bool) if self.clock is None else self.clock


class Ambiguous(Exception):
    pass


# ------------------------------------------------------------------------------------------- the cases
def _rng(seed):
    return np.random.default_rng(seed)


def _rows_of(keys, times, seed):
    """every key `times` times, shuffled"""
    return _rng(seed).permutation(np.tile(np.array(keys, np.int64), times))


def _chain_mid():
    return Case("chain_mid", _rows_of(chain_keys(MID, 600), 3, 1), chunk=500)


def _wrap_rows():
    chain = chain_keys(LAST, 300)
    displaced = [chain_keys(h, 1, first=5)[0] for h in range(300)]      # their own homes are slots 0..299
    return _rows_of(chain + displaced, 3, 2)


def _chain_wrap():
    return Case("chain_wrap", _wrap_rows(), chunk=500)


def _chain_two():
    a, b = chain_keys(MID, 300), chain_keys(MID + 1, 300)
    ab = np.array([k for pair in zip(a, b) for k in pair], np.int64)     # interleaved row by row
    return Case("chain_two", np.concatenate([ab, ab[::-1], ab]), chunk=512)


def _sentinel_first():
    others = list(NEIGHBOURS) + spread_keys(40, 3)
    head = np.array([I64_MIN] + others, np.int64)
    return Case("sentinel_first", np.concatenate([head, _rows_of([I64_MIN] + others, 2, 3)]), chunk=32)


def _sentinel_only():
    """the first push is the sentinel alone, in three chunks; the neighbours arrive in the second push"""
    second = np.array([k for n in NEIGHBOURS for k in (n, I64_MIN)] * 3, np.int64)
    return Case("sentinel_only", np.concatenate([np.full(300, I64_MIN, np.int64), second]), chunk=128, cuts=(300,))


def _late_rows():
    others = list(NEIGHBOURS) + spread_keys(60, 4)
    base = _rows_of(others, 6, 4)                         # 390 rows without the sentinel
    return np.insert(base, [150, 200, 300, 388], I64_MIN)    # rows 150 (the third 64-row chunk), 201, 302 and 391


def _sentinel_late():
    return Case("sentinel_late", _late_rows(), chunk=64, cuts=(300,))


def _dup_heavy():
    """40 keys, about 200 rows each, new in one 8000-row chunk: first occurrences in descending raw value, key 0 first
    at row 0 and key 39 first at the chunk's last row; a second chunk brings every key once more"""
    keys = np.array(sorted(spread_keys(40, 5), reverse=True), np.int64)
    n = 8000
    intro = {0: 0, n - 1: 39}
    intro.update({200 * i: i for i in range(1, 39)})
    rng, rows, seen = _rng(5), np.zeros(n, np.int64), 0
    for r in range(n):
        if r in intro:
            rows[r], seen = keys[intro[r]], intro[r] + 1
        else:
            rows[r] = keys[rng.integers(0, seen)]
    return Case("dup_heavy", np.concatenate([rows, keys[::-1]]), chunk=n)


def _chunk_edges():
    """pushes (one chunk each) of 1, 255, 256 and 257 rows: one new key alone; every row a new key; no new key at all
    (kd_resolve's m == 0 return); new and known keys mixed"""
    a = spread_keys(1, 6)
    b = spread_keys(255, 7)
    c = spread_keys(100, 8)
    p3 = _rows_of(a + b, 1, 6)
    p4 = _rng(7).permutation(np.array(c * 2 + b[:57], np.int64))
    return Case("chunk_edges", np.concatenate([np.array(a + b, np.int64), p3, p4]), chunk=300, cuts=(1, 256, 512))


def _pushes_chain():
    rows = _wrap_rows()
    return Case("pushes_chain", rows, chunk=250, cuts=(len(rows) // 3, 2 * len(rows) // 3))


def _pushes_sentinel():
    return Case("pushes_sentinel", _late_rows(), chunk=64, cuts=(155, 300))


def _clock_rows():
    """every seventh row is clock-only (stream -1): no key, though its raw value is one no other row has"""
    keyed = _rows_of(spread_keys(50, 9), 3, 9)
    clock = np.arange(len(keyed) * 7 // 6) % 7 == 3
    raw = np.full(len(clock), 777, np.int64)
    raw[~clock] = keyed
    return Case("clock_rows", raw, chunk=40, clock=clock)


def _grow_first(s, keys=None, name="grow_first"):
    """1000 new keys per shard in the first chunk: one rebuild (1024 -> 4096)"""
    keys = keys if keys is not None else spread_keys(1000 * s, 10)
    first = _rng(10).permutation(np.array(keys, np.int64))
    return Case(name, np.concatenate([first, _rows_of(keys, 1, 11)]), chunk=len(keys), cap0=SMALL_CAP, scale=s)


def _grow_twice(s):
    """3300 new keys per shard in one chunk: past 1024 and past 4096 with every thread's overshoot (2048 + 1024)"""
    keys = spread_keys(3300 * s, 12)
    first = _rng(12).permutation(np.array(keys, np.int64))
    return Case("grow_twice", np.concatenate([first, _rows_of(keys, 1, 13)]), chunk=len(keys), cap0=SMALL_CAP, scale=s)


def _grow_late(s, sentinel_chunk=None, name="grow_late"):
    """chunks of 450 rows per shard.  Chunks 0-4 bring 90 new keys per shard each (450: under the limit of 512), chunk
    5 brings 420 (870: past 512 + 256) and rebuilds with 450 assigned keys to rehash; then every key comes again.
    sentinel_chunk: one of the chunk's new keys is the sentinel."""
    C = 450 * s
    keys = spread_keys(870 * s, 14)
    rng, rows, lo = _rng(14), [], 0
    for j in range(6):
        m = (90 if j < 5 else 420) * s
        new = list(keys[lo:lo + m])
        if sentinel_chunk == j:
            new[m // 2] = I64_MIN
            keys[lo + m // 2] = I64_MIN
        lo += m
        fill = rng.choice(np.array(keys[:lo], np.int64), C - m)
        if sentinel_chunk is not None and j > sentinel_chunk:
            fill[::50] = I64_MIN
        chunk = np.concatenate([np.array(new, np.int64), fill])
        rows.append(np.concatenate([chunk[:1], rng.permutation(chunk[1:])]))
    rows.append(_rows_of(keys, 1, 15))
    return Case(name, np.concatenate(rows), chunk=C, cap0=SMALL_CAP, scale=s)


def _reset_after_growth(s):
    """a growth stream, a reset, then half of its keys in another order with new ones between them"""
    first = _grow_first(s)
    old = spread_keys(1000 * s, 10)[::2][::-1]
    second = _rows_of(old + spread_keys(300 * s, 16), 2, 16)
    n1 = len(first.raw)
    return Case("reset_after_growth", np.concatenate([first.raw, second]), chunk=first.chunk, cuts=(n1,),
                cap0=SMALL_CAP, reset_at=n1, scale=s)


PLAIN = {
    "chain_mid": _chain_mid, "chain_wrap": _chain_wrap, "chain_two": _chain_two, "sentinel_first": _sentinel_first,
    "sentinel_only": _sentinel_only, "sentinel_late": _sentinel_late, "dup_heavy": _dup_heavy,
    "chunk_edges": _chunk_edges, "pushes_chain": _pushes_chain, "pushes_sentinel": _pushes_sentinel,
    "clock_rows": _clock_rows,
}
GROWTH = {
    "grow_first": _grow_first, "grow_twice": _grow_twice, "grow_late": _grow_late,
    "grow_sentinel_kept": lambda s: _grow_late(s, 0, "grow_sentinel_kept"),
    "grow_sentinel_pending": lambda s: _grow_late(s, 5, "grow_sentinel_pending"),
    "grow_chain": lambda s: _grow_first(s, chain_keys(LAST, 1000 * s), "grow_chain"),
    "reset_after_growth": _reset_after_growth,
}
# home slot of the chain keys of a case (every capacity the case runs through is checked by the guard)
CHAINS = {"chain_mid": [MID], "chain_wrap": [LAST], "chain_two": [MID, MID + 1], "pushes_chain": [LAST],
          "grow_chain": [LAST]}


@functools.lru_cache(maxsize=None)
def case(name: str, scale: int = 1) -> Case:
    """the case; growth cases are sized per shard (`scale` = the number of shards they run on)"""
    if name in PLAIN:
        assert scale == 1
        return PLAIN[name]()
    return GROWTH[name](scale)


# ------------------------------------------------------------------------------------------- the reference
def pieces(c: Case) -> List[Tuple[int, int]]:
    cuts = [0] + list(c.cuts) + [len(c.raw)]
    return list(zip(cuts[:-1], cuts[1:]))


def streams(c: Case) -> List[Tuple[int, int]]:
    """row ranges between resets"""
    return [(0, len(c.raw))] if c.reset_at is None else [(0, c.reset_at), (c.reset_at, len(c.raw))]


def chunks(c: Case) -> List[Tuple[int, int]]:
    """the chunks the node cuts the pushes into"""
    return [(a, min(a + c.chunk, hi)) for lo, hi in pieces(c) for a in range(lo, hi, c.chunk)]


def ref_ids(c: Case) -> np.ndarray:
    """first-seen dense id of every row's key (-1: a clock-only row), row at a time"""
    ids, clock = np.full(len(c.raw), -1, np.int32), c.is_clock()
    for lo, hi in streams(c):
        seen: Dict[int, int] = {}
        for r in range(lo, hi):
            if not clock[r]:
                ids[r] = seen.setdefault(int(c.raw[r]), len(seen))
    return ids


def distinct_after(c: Case, hi: int) -> int:
    """distinct keys of the stream that holds row hi - 1, up to that row"""
    lo = max(a for a, b in streams(c) if a < hi)
    return len(set(c.raw[lo:hi][~c.is_clock()[lo:hi]].tolist()))


def batch(c: Case, lo: int, hi: int, base: int, key=None) -> Batch:
    """rows [lo, hi) of a stream that starts at row `base`, as the query's batch (id, symbol, price)"""
    n = hi - lo
    row = np.arange(lo - base, hi - base, dtype=np.int64)
    clock = c.is_clock()[lo:hi]
    key = (ref_ids(c)[lo:hi] if key is None else key).astype(np.int32)
    return Batch(n, lo - base, 1_700_000_000_000 + row // 32, np.where(clock, -1, 0).astype(np.int32), key,
                 [row.copy(), key.copy(), (21 + 0.25 * row).astype(np.float32)], [None] * 3)


@functools.lru_cache(maxsize=None)
def want(name: str, scale: int = 1) -> Tuple[Outputs, ...]:
    """the oracle engine over the reference's dense ids: one Outputs per stream (between resets).  Shared; no test
    changes it."""
    from oracle import OracleEngine
    from parity_util import run_engine
    c = case(name, scale)
    return tuple(run_engine(OracleEngine, QUERY, [batch(c, lo, hi, lo)]) for lo, hi in streams(c))


# ------------------------------------------------------------------------------------------- the table's model
def shard_of(raw: np.ndarray, gpus: int) -> np.ndarray:
    """the shard of every row (the product's router hash)"""
    return (mix64(np.ascontiguousarray(raw, np.int64)) % np.uint64(gpus)).astype(np.int64)


def model(c: Case, gpus: int = 1, rule: str = "first_seen"):
    """The dictionaries of `gpus` shards over the case's chunks: (per-row ids, per-shard stats).  The ids follow
    `rule` (gpus == 1 only): "first_seen" is the right one, RULES are plausible wrong ones.  Stats: cap, n_keys,
    rebuilds and probes per shard, as sg_node_key_dict_stats reports them after the last push.  Raises Ambiguous where
    a rebuild would depend on timing."""
    assert rule == "first_seen" or (rule in RULES and gpus == 1)
    n, clock = len(c.raw), c.is_clock()
    shard = shard_of(c.raw, gpus)
    ids = np.full(n, -1, np.int64)
    st = [dict(cap=0, n_keys=0, rebuilds=0, probes=0) for _ in range(gpus)]
    known: List[Dict[int, int]] = [dict() for _ in range(gpus)]
    resets = {c.reset_at}
    for lo, hi in chunks(c):
        if lo in resets:
            for s in range(gpus):
                known[s], st[s]["n_keys"] = {}, 0
        for s in range(gpus):
            # G = 1 resolves the chunk as it is; the exchange drops clock-only rows before the shards see them
            rows = [r for r in range(lo, hi) if shard[r] == s and (gpus == 1 or not clock[r])]
            if not rows:
                continue
            t, d = st[s], known[s]
            if t["cap"] == 0:
                t["cap"] = c.cap0
            keyed = [r for r in rows if not clock[r]]

            def new_keys():
                first, last = {}, {}
                for r in keyed:
                    k = int(c.raw[r])
                    if k not in d:
                        first.setdefault(k, r)
                        last[k] = r
                return first, last
            first, last = new_keys()
            t["probes"] += 1
            while t["n_keys"] + len(first) >= t["cap"] // 2:
                if t["n_keys"] + len(first) <= t["cap"] // 2 + probe_threads(t["cap"], len(rows)):
                    raise Ambiguous(f"{c.name} G={gpus} shard {s} chunk at {lo}: {t['n_keys']} + {len(first)} keys, "
                                    f"cap {t['cap']}")
                t["cap"] *= 4
                t["rebuilds"] += 1
                t["probes"] += 1
                if rule == "sentinel_fresh" and I64_MIN in d:     # (a rebuild that forgets the sentinel's id)
                    del d[I64_MIN]
                    first, last = new_keys()
            order = {"first_seen": lambda k: first[k], "sentinel_fresh": lambda k: first[k],
                     "per_chunk": lambda k: first[k], "ascending_raw": lambda k: k,
                     "slot_order": lambda k: (kd_home(k, t["cap"]), k), "last_occurrence": lambda k: last[k]}[rule]
            base = 0 if rule == "per_chunk" else t["n_keys"]
            for rank, k in enumerate(sorted(first, key=order)):
                d[k] = base + rank
            t["n_keys"] += len(first)
            for r in keyed:
                ids[r] = d[int(c.raw[r])]
    return ids, st
