"""tests/name_table_cases.py on the CPU: the hash restated twice agrees with itself, the pool's ids home where the GPU tests
need them, and the chains those tests rely on — a block across the table's last slot, walks below and beyond the parser's
1025 slots — are there by simulation, whatever order the ids are inserted in."""
import numpy as np
import pytest

import name_table_cases as nt

CAP = nt.PARSER_MIN_CAP


@pytest.fixture(scope="module")
def pool():
    return nt.pool(1400)


def test_vectorised_hash_equals_the_scalar_one():
    rng = np.random.default_rng(20250311)
    for length in [0, 1, 2, 7, 8, 9, 63, 64, 299, 300] + rng.integers(0, 301, 20).tolist():
        rows = rng.integers(0, 256, (25, length), dtype=np.uint8)
        got = nt.gp_hash(rows)
        assert got.dtype == np.uint64 and got.tolist() == [nt.gp_hash_scalar(r.tobytes()) for r in rows], length
    # two values worked out by hand from csrc/gpu_text.h: the empty id is the seed mixed; length enters the seed
    assert nt.gp_hash_scalar(b"") == (lambda h: (h ^ (h >> 32)))((((0xcbf29ce484222325 ^ (0xcbf29ce484222325 >> 29)) * 0xbf58476d1ce4e5b9) & (2**64 - 1)))
    assert nt.gp_hash_scalar(b"\0") != nt.gp_hash_scalar(b"\0\0")


def test_pool_ids_are_distinct_plain_and_home_into_the_last_256_slots(pool):
    assert len(set(pool)) == 1400 and all(len(x) == 8 and x[:1] == b"p" and set(x[1:]) <= set(nt.ALPHABET) for x in pool)
    assert not set(b"".join(pool)) & set(b"\t \"\r\n")
    assert nt.pool(10) == pool[:10]  # a fixed enumeration: asking again, or for fewer, gives the same ids
    for cap in (1024, 2048, 4096, CAP):
        h = nt.homes(pool, cap)
        assert h.min() >= cap - nt.HOME_WINDOW and h.max() < cap, cap
        assert h.tolist() == [nt.gp_hash_scalar(x) & (cap - 1) for x in pool]


def _orders(K, seed):
    rng = np.random.default_rng(seed)
    return [np.arange(K)] + [rng.permutation(K) for _ in range(3)]


def test_first_900_ids_are_one_block_across_the_end_and_no_walk_outgrows_it(pool):
    ids = pool[:900]
    first = int(nt.homes(ids, CAP).min())
    for order in _orders(900, 1):
        mask, examined = nt.occupied(ids, CAP, order.tolist())
        assert nt.clusters(mask) == [(first, 900)] and nt.wraps(mask)
        assert np.array_equal(mask, nt.occupied_mask(nt.homes(ids, CAP), CAP))  # the occupied set does not depend on the order
        assert 900 - 255 <= examined.max() <= 900 < nt.WALK_SLOTS
        print("K = 900: the longest walk looks at %d slots" % examined.max())
    # with the plain ids of case (a) beside them no chain reaches the bound either, wherever those land
    assert nt.longest_cluster(nt.occupied_mask(nt.homes(nt.chain_ids(), CAP), CAP)) < nt.WALK_SLOTS


def test_1400_ids_force_a_walk_beyond_1025_slots_in_every_order(pool):
    first = int(nt.homes(pool, CAP).min())
    for order in _orders(1400, 2):
        mask, examined = nt.occupied(pool, CAP, order.tolist())
        assert nt.clusters(mask) == [(first, 1400)] and nt.wraps(mask)
        # the id that ends in the block's last slot homes in front of the table's end: it has looked at 1400 - 255 slots at least
        assert examined.max() >= 1400 - 255 > nt.WALK_SLOTS
        print("K = 1400: the longest walk looks at %d slots" % examined.max())


@pytest.mark.parametrize("K,cap", [(400, 1024), (600, 2048), (1400, 4096)])
def test_small_tables_hold_a_cluster_across_the_end(pool, K, cap):
    assert nt.pow2_cap(K) == cap
    mask, _ = nt.occupied(pool[:K], cap)
    assert nt.wraps(mask) and nt.longest_cluster(mask) == K and int(mask.sum()) == K


def test_natural_ids_at_the_highest_legal_load_stay_far_below_the_bound():
    ids = nt.distinct_ids(524288)
    assert nt.parser_holds_comfortably(len(ids), CAP) and not nt.parser_holds_comfortably(len(ids) + 1, CAP)
    for n in (524288, 524289):  # a walk never leaves its cluster: the longest cluster bounds every walk, in every order
        longest = nt.longest_cluster(nt.occupied_mask(nt.homes(nt.distinct_ids(n), CAP), CAP))
        print("%d plain ids in 2^20 slots: the longest cluster has %d slots" % (n, longest))
        assert longest < nt.WALK_SLOTS


def test_size_rules():
    assert nt.parser_cap(0) == nt.parser_cap(64 << 20) == CAP and nt.parser_cap((64 << 20) + 64) == 2 * CAP
    assert nt.parser_cap(nt.SEGMENT + 63) == 2 * CAP and nt.parser_cap(nt.SEGMENT + 64) == 4 * CAP
    assert [nt.pow2_cap(n) for n in (0, 512, 513, 600, 900, 1024, 1025, 1420)] == [1024, 1024, 2048, 2048, 2048, 2048, 4096, 4096]
    assert nt.parser_holds_comfortably(1024, 1024) and nt.parser_holds_comfortably(1400, CAP)
    assert nt.range_cuts(3 * 32768, 3) == [0, 32768, 65536, 98304] and nt.range_cuts(3 * 32768 + 1, 3) == [0, 65536, 98305, 98305]


def test_the_texts_name_every_id_twice_and_the_large_ones_are_what_they_say(pool):
    for m4 in (False, True):
        text = nt.overlap_text(nt.chain_ids(), m4)
        delim, ib = (b" ", 1) if m4 else (b"\t", 5)
        firsts = [l.split(delim)[0] for l in text.splitlines()]
        assert all(firsts.count(x) == 2 for x in nt.chain_ids())
        assert len(text.splitlines()[0].split(delim)) == 12
    text = nt.distinct_text(1001)
    names = [f for l in text.splitlines() for f in (l.split(b"\t")[0], l.split(b"\t")[5])]
    assert sorted(names) == sorted(nt.distinct_ids(1001) + [b"r0"]) and text.count(b"\n") == 501
    text = nt.read_to_reference(1000)
    assert len({l.split(b"\t")[0] for l in text.splitlines()}) == 1000 and {l.split(b"\t")[5] for l in text.splitlines()} == {b"ref"}
    for n, late in ((2, ()), (3, ()), (3, tuple(pool[300:305]))):
        text = nt.merge_text(n, pool[:300], late)
        cuts = nt.range_cuts(len(text), n)
        seen = nt.ids_per_range(text, cuts)
        assert len(text) == n * nt.RANGE_BYTES and cuts == [k * nt.RANGE_BYTES for k in range(n + 1)]
        assert [len(s) for s in seen] == [300] * (n - 1) + [300 + len(late)] and all(set(pool[:300]) <= s for s in seen)
        assert nt.pow2_cap(sum(len(s) for s in seen)) == 2048


def test_editor_tables_and_their_close_ids():
    (a, b, c), (p, px, py) = nt.close_ids()
    assert a[:7] == b[:7] == c[:7] and len({a, b, c}) == 3 and px[:8] == py[:8] == p and len(px) == len(py) == 10 and px != py
    assert a in nt.pool(2200) and b in nt.pool(2200) and p in nt.pool(1)
    assert min(nt.homes([a, b, c, p, px, py], 1024)) >= 768
    for small, (names, types) in ((True, nt.small_table()), (False, nt.large_table())):
        cap = nt.pow2_cap(len(names))
        assert cap == (1024 if small else 4096) and set(types) == {0, 1, 2} and len(set(names)) == len(names)
        mask, _ = nt.occupied(names, cap)
        chain = max(nt.clusters(mask), key=lambda c: c[1])
        assert nt.wraps(mask) and chain[1] >= (400 if small else 1400) and chain[0] + chain[1] > cap
        # an absent pool id homes inside the chain: its miss ends at the chain's far end, behind the wrap
        absent = nt.absent_pool_ids(names)
        assert len(absent) == 300 and not set(absent) & set(names)
        assert all(mask[h] and h >= chain[0] for h in nt.homes(absent + ([c, py] if small else []), cap))
        named = nt.lookup_ids(names, small)
        assert set(names) < set(named) and set(nt.PLAIN_ABSENT) <= set(named) - set(names)


def test_walk_cases_are_exact():
    for walk in (nt.WALK_SLOTS, nt.WALK_SLOTS + 1):
        text, K, x = nt.walk_case(walk)  # (asserts the walk by simulation)
        assert len(text) > nt.SEGMENT and text.rindex(b"\n" + x + b"\t") + 1 >= nt.SEGMENT and text.index(x + b"\t") >= nt.SEGMENT
        assert K + 1 < 2048  # 2 R <= cap by far: only the walk decides
