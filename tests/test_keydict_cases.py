"""CPU guard of the key dictionary cases (keydict_cases.py): the cases are what they claim, before test_keydict_gpu.py
relies on them.  No GPU."""
import numpy as np
import pytest

import keydict_cases as KC

ALL = [(n, 1) for n in KC.PLAIN] + [(n, s) for n in KC.GROWTH for s in (1, 2)]
IDS = [f"{n}-x{s}" for n, s in ALL]

# The wrong rules each case is there to tell from first-seen order ("the test says which"): every case names at least
# one, every rule is named by at least one case, and the guard checks each claim on the model's ids.
#   ascending_raw    new keys of a chunk numbered by ascending raw value
#   slot_order       ... by home slot (then raw value): the order a scan of the table would give
#   last_occurrence  ... by their last row in the chunk instead of their first
#   per_chunk        ids restart at 0 in every chunk (the base n_keys forgotten)
#   sentinel_fresh   a rebuild forgets the sentinel's id; its next row gets a new one
SEPARATES = {
    "chain_mid": ("ascending_raw", "slot_order", "last_occurrence", "per_chunk"),
    "chain_wrap": ("ascending_raw", "slot_order", "per_chunk"),
    "chain_two": ("ascending_raw", "slot_order", "last_occurrence", "per_chunk"),
    "sentinel_first": ("slot_order", "last_occurrence", "per_chunk"),
    "sentinel_only": ("ascending_raw", "per_chunk"),
    "sentinel_late": ("ascending_raw", "per_chunk"),
    "dup_heavy": ("ascending_raw", "last_occurrence"),
    "chunk_edges": ("ascending_raw", "per_chunk"),
    "pushes_chain": ("ascending_raw", "per_chunk"),
    "pushes_sentinel": ("ascending_raw", "per_chunk"),
    "clock_rows": ("ascending_raw", "per_chunk"),
    "grow_first": ("ascending_raw", "slot_order"),
    "grow_twice": ("ascending_raw", "slot_order"),
    "grow_late": ("ascending_raw", "per_chunk"),
    "grow_sentinel_kept": ("sentinel_fresh", "per_chunk"),
    "grow_sentinel_pending": ("ascending_raw", "per_chunk"),
    "grow_chain": ("ascending_raw", "slot_order"),
    "reset_after_growth": ("ascending_raw", "last_occurrence"),
}


def test_every_rule_and_every_case_is_covered():
    assert set(SEPARATES) == set(KC.PLAIN) | set(KC.GROWTH)
    assert all(SEPARATES.values())
    assert {r for rs in SEPARATES.values() for r in rs} == set(KC.RULES)


def test_python_hash_restatement():
    """INV inverts the multiplier; the chain construction lands on its slot at every capacity"""
    assert (KC.M * KC.INV) & KC.MASK == 1
    for home in (0, 1, KC.MID, KC.LAST):
        for k in KC.chain_keys(home, 50):
            for c in range(10, 23):
                assert KC.kd_home(k, 1 << c) == home >> (22 - c)
    assert len(set(KC.chain_keys(KC.LAST, 4000))) == 4000 and KC.I64_MIN not in KC.chain_keys(KC.LAST, 4000)


@pytest.mark.parametrize("name,scale", ALL, ids=IDS)
def test_case_is_what_it_claims(name, scale):
    c = KC.case(name, scale)
    keyed = c.raw[~c.is_clock()]
    # every key has two rows or more, in its stream (between resets)
    for lo, hi in KC.streams(c):
        _, counts = np.unique(c.raw[lo:hi][~c.is_clock()[lo:hi]], return_counts=True)
        assert counts.min() >= 2
    # the cuts are push boundaries in order; a reset falls on one
    assert list(c.cuts) == sorted(set(c.cuts)) and all(0 < x < len(c.raw) for x in c.cuts)
    assert c.reset_at is None or c.reset_at in c.cuts
    # the model's first-seen ids are the row-at-a-time dictionary's, and no rebuild depends on timing, on every route
    if scale == 1:
        assert np.array_equal(KC.model(c, 1)[0], KC.ref_ids(c))
    st = KC.model(c, scale)[1]
    routes = (scale,) if name in KC.GROWTH else (1, 2, 3)
    for g in routes:
        _, sg = KC.model(c, g)                                  # (raises Ambiguous)
        if name in KC.GROWTH:
            assert all(t["rebuilds"] >= 1 and t["cap"] > KC.SMALL_CAP for t in sg), (g, sg)
        else:
            assert all(t["rebuilds"] == 0 and t["cap"] == KC.KD_MIN_CAP for t in sg), (g, sg)
    # chains: one home slot at every capacity the case runs through; the wrap cases' home is the last slot
    caps = {c.cap0 << (2 * k) for k in range(st[0]["rebuilds"] + 1)}
    assert max(caps) == st[0]["cap"]
    if name in KC.CHAINS:
        for cap in caps:
            shift = 22 - (cap.bit_length() - 1)
            homes = {KC.kd_home(int(k), cap) for k in keyed}
            want = {h >> shift for h in KC.CHAINS[name]}
            if name in ("chain_wrap", "pushes_chain"):           # (plus the displaced keys of slots 0..299)
                assert homes == want | {h >> shift for h in range(300)}
            else:
                assert homes == want
            if KC.LAST in KC.CHAINS[name]:
                assert cap - 1 in want


def test_named_sizes():
    """what the docstrings of the cases say, read off their rows"""
    assert KC.model(KC.case("grow_twice"), 1)[1][0] == dict(cap=16384, n_keys=3300, rebuilds=2, probes=4)
    assert KC.model(KC.case("grow_first"), 1)[1][0] == dict(cap=4096, n_keys=1000, rebuilds=1, probes=3)
    late = KC.case("grow_late")
    for name, first_chunk in (("grow_sentinel_kept", 0), ("grow_sentinel_pending", 5)):
        c = KC.case(name)
        r = int(np.nonzero(c.raw == KC.I64_MIN)[0][0])
        assert r // c.chunk == first_chunk and np.any(c.raw[6 * c.chunk:] == KC.I64_MIN)
    # the rebuild of grow_late comes in its sixth chunk, with 450 assigned keys to carry
    five = KC.Case("five", late.raw[:5 * late.chunk], chunk=late.chunk, cap0=KC.SMALL_CAP)
    assert KC.model(five, 1)[1][0] == dict(cap=1024, n_keys=450, rebuilds=0, probes=5)
    six = KC.Case("six", late.raw[:6 * late.chunk], chunk=late.chunk, cap0=KC.SMALL_CAP)
    assert KC.model(six, 1)[1][0] == dict(cap=4096, n_keys=870, rebuilds=1, probes=7)
    s = KC.case("sentinel_first")
    assert s.raw[0] == KC.I64_MIN
    s = KC.case("sentinel_only")
    assert set(s.raw[:300].tolist()) == {KC.I64_MIN} and set(KC.NEIGHBOURS) < set(s.raw[300:].tolist())
    s = KC.case("sentinel_late")
    first = int(np.nonzero(s.raw == KC.I64_MIN)[0][0])
    assert first // s.chunk == 2 and np.any(s.raw[s.cuts[0]:] == KC.I64_MIN)
    for n in ("sentinel_first", "sentinel_late", "pushes_sentinel"):
        assert set(KC.NEIGHBOURS) < set(KC.case(n).raw.tolist())
    d = KC.case("dup_heavy")
    firsts = {int(k): int(np.nonzero(d.raw == k)[0][0]) for k in np.unique(d.raw)}
    by_first = sorted(firsts, key=firsts.get)
    assert len(firsts) == 40 and by_first == sorted(firsts, reverse=True)
    assert firsts[by_first[0]] == 0 and firsts[by_first[-1]] == d.chunk - 1
    e = KC.case("chunk_edges")
    assert [hi - lo for lo, hi in KC.chunks(e)] == [1, 255, 256, 257]
    ids = KC.ref_ids(e)
    new = [len(set(ids[lo:hi].tolist()) - set(ids[:lo].tolist())) for lo, hi in KC.chunks(e)]
    assert new == [1, 255, 0, 100]
    r = KC.case("reset_after_growth")
    a, b = set(r.raw[:r.reset_at].tolist()), set(r.raw[r.reset_at:].tolist())
    assert len(a & b) == 500 and len(b - a) == 300 and len(a) == 1000
    assert KC.model(r, 1)[1][0] == dict(cap=4096, n_keys=800, rebuilds=1, probes=5)
    k = KC.case("clock_rows")
    assert k.is_clock().sum() > 10 and 777 not in set(k.raw[~k.is_clock()].tolist())


@pytest.mark.parametrize("name,scale", ALL, ids=IDS)
def test_oracle_shows_every_key_and_every_wrong_rule_named(name, scale):
    """100 % of the keys of every case are the key of at least one match in the oracle's output, so a wrong id of any
    key is visible; and the ids of each wrong rule the case names differ from the right ones on such a key."""
    c = KC.case(name, scale)
    ids = KC.ref_ids(c)
    outs = KC.want(name, scale)
    for (lo, hi), w in zip(KC.streams(c), outs):
        keys = set(ids[lo:hi][~c.is_clock()[lo:hi]].tolist())
        assert set(w.key.tolist()) == keys and len(keys) == KC.distinct_after(c, hi)
        n_keyed = int((~c.is_clock()[lo:hi]).sum())
        assert len(w) == n_keyed - len(keys)                   # a key with r rows emits r - 1 matches
        # a match's key is the reference id of the raw key of its trigger row
        assert np.array_equal(w.key, ids[lo + w.trigger.astype(np.int64)])
    if scale == 1:
        for rule in KC.RULES:
            wrong, _ = KC.model(c, 1, rule)
            assert (rule in SEPARATES[name]) <= bool(np.any(wrong != ids)), rule
