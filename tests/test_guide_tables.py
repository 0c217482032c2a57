"""The guided-decoding arena's allocator (``engine.GuideTables``): host
bookkeeping of which guide tables are resident and where, without a device.
Its contract is the class's docstring; a slip here would overwrite a table a
running request reads. The device side is covered by tests/test_gpu_guided.py."""
import random

import pytest

from p2p_llm_tunnel_amd.models.engine import GuideTables


def spans(t):
    return sorted((first, first + rows) for first, rows, _, _ in t.tables.values())


def test_a_shared_key_uploads_once_and_counts_two_holders():
    t = GuideTables(16)
    assert t.reserve("a", 5) == (0, True)
    assert t.reserve("a", 5) == (0, False)
    assert t.tables["a"][:3] == [0, 5, 2]
    t.release("a")
    assert t.tables["a"][2] == 1


def test_an_idle_table_is_found_resident_again():
    t = GuideTables(16)
    t.reserve("a", 5)
    t.release("a")
    assert t.tables["a"][2] == 0  # idle, still there
    assert t.reserve("b", 4) == (5, True)
    assert t.reserve("a", 5) == (0, False)


def test_a_freed_gap_in_the_middle_is_reused_first_fit():
    t = GuideTables(16)
    for key in "abc":
        assert t.reserve(key, 4) == ("abc".index(key) * 4, True)
    t.release("b")
    assert t.reserve("d", 5) is None  # 4 rows at the end, 4 in the middle once b goes: never 5 together
    assert "b" in t.tables
    assert t.reserve("e", 4) == (12, True)  # the first gap that is free now
    assert t.reserve("f", 3) == (4, True)  # no room left beside b: b goes, and its gap is taken from its start
    assert "b" not in t.tables and spans(t) == [(0, 4), (4, 7), (8, 12), (12, 16)]
    assert t.reserve("g", 1) == (7, True)


def test_the_least_recently_used_idle_table_is_evicted():
    t = GuideTables(12)
    for key in "abc":
        t.reserve(key, 4)
    for key in "abc":
        t.release(key)
    assert t.reserve("a", 4) == (0, False)  # a is used again: b is now the oldest
    t.release("a")
    assert t.reserve("d", 4) == (4, True)
    assert sorted(t.tables) == ["a", "c", "d"]
    assert t.reserve("e", 4) == (8, True)  # then c; a, touched last, stays
    assert sorted(t.tables) == ["a", "d", "e"]


def test_an_idle_table_stays_when_a_gap_already_fits():
    t = GuideTables(16)
    t.reserve("a", 4)
    t.release("a")
    assert t.reserve("b", 12) == (4, True)
    assert "a" in t.tables and t.tables["a"][:3] == [0, 4, 0]


def test_no_room_beside_the_held_tables_evicts_nothing():
    t = GuideTables(16)
    t.reserve("idle", 4)
    t.reserve("held", 4)
    t.release("idle")
    before = {k: v[:3] for k, v in t.tables.items()}
    assert t.reserve("big", 13) is None  # 8 rows together at most, even with the idle table gone
    assert {k: v[:3] for k, v in t.tables.items()} == before
    assert t.reserve("fits", 8) == (8, True) and "idle" in t.tables  # the tail is free: nothing has to go
    t.release("held")
    assert t.reserve("big", 9) is None and sorted(t.tables) == ["fits", "held", "idle"]  # still only 8 beside fits


def test_the_arena_size_fits_an_empty_arena_and_one_more_never_does():
    t = GuideTables(16)
    assert t.reserve("all", 16) == (0, True)
    t.release("all")
    assert t.reserve("more", 17) is None and "all" in t.tables
    assert t.reserve("one", 1) == (0, True) and "all" not in t.tables
    assert GuideTables(16).reserve("more", 17) is None
    for bad in (0, -1, True, 1.5, 1 << 15):
        with pytest.raises(ValueError, match="guided_states"):
            GuideTables(bad)


def test_random_soak_keeps_the_invariants():
    rng = random.Random(7)
    S = 64
    t = GuideTables(S)
    sizes = {k: rng.choice((1, 2, 3, 5, 8, 13, 21, 40, 64)) for k in range(24)}
    holders = {}  # key -> outstanding reserves
    rows = {}  # held key -> the first row it was given
    refused = 0
    for _ in range(4000):
        held = [k for k, n in holders.items() if n]
        if held and rng.random() < 0.5:
            k = rng.choice(held)
            t.release(k)
            holders[k] -= 1
            if not holders[k]:
                del rows[k]
        else:
            k = rng.randrange(len(sizes))
            was = k in t.tables
            got = t.reserve(k, sizes[k])
            if got is None:
                refused += 1
                assert not was
            else:
                assert got[1] == (not was)
                holders[k] = holders.get(k, 0) + 1
                rows.setdefault(k, got[0])
        sp = spans(t)
        assert all(0 <= a < b <= S for a, b in sp) and all(x[1] <= y[0] for x, y in zip(sp, sp[1:]))
        assert all(t.tables[k][0] == first and t.tables[k][1] == sizes[k] for k, first in rows.items())
        assert {k: v[2] for k, v in t.tables.items() if v[2]} == {k: n for k, n in holders.items() if n}
    assert refused and len(t.tables) > 1  # both outcomes were exercised
