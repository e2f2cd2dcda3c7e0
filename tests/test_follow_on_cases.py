"""tests/follow_on_cases.py's reads do what they say (no GPU): every claim is held against the CPU emulations of
tests/formulation.py at the long-batch follow-on's instantiation (filtered_sweep_regions: 32 coarse blocks, windows of 32, 128 kept
events; the screen: slid_window_screen_regions without a slide) and against the oracle; the set as a whole stands on both sides of
every guard."""
import numpy as np
import pytest

import follow_on_cases as fc
import formulation
import oracle


def oracle_regions(iv, L, c):
    a = np.array(iv, dtype=np.uint32).reshape(-1, 2)
    _, br, _ = oracle.run(np.array([0, len(a)], np.uint64), a, np.array([L], np.uint64), c, 0.4, n_threads=1)
    return [tuple(x) for x in br.tolist()]


def check_case(k, c):
    """the three things every case owes: the emulation equals the oracle where it decides; the case is on the side of its guard
    that it claims; the screen defers it (or, for n <= c, answers itself)"""
    ctx = (k.name, c)
    got, m = fc.filtered(k.iv, k.L, c)
    assert (got is not None) == (k.claim == "decided"), ctx
    if got is not None:
        assert got == oracle_regions(k.iv, k.L, c), ctx
    if k.m is not None:
        assert m == k.m, (ctx, m)
    assert fc.screen_defers(k.iv, k.L, c) == k.defer, ctx
    t = fc.table(k.iv, k.L)
    cc = min(c, 0x3FFFFFFF)
    assert 65 <= t["n"] <= 256 and t["pmax"] <= k.L, ctx
    # one guard at a time: a case that is left is on the wrong side of ITS guard alone
    fails = {"n": t["n"] <= cc, "F": t["F"] <= cc, "G": t["G"] <= cc, "length": t["tmin"] < fc.W, "cap": m is not None and m > fc.CAP}
    if k.claim == "left":
        # (a read of n <= c intervals cannot have F > c either: the guard in front answers; at c = n - 1 a chimera — half of
        #  its starts at the head, half of its ends at the tail — has neither F > c nor G > c)
        also = {"F", "G"} if k.guard == "n" else {"G"} if k.name.startswith("c = n - 1") else set()
        expect = {g for g in fails if fails[g]} - also
        assert expect == {k.guard}, (ctx, fails)
    else:
        assert not any(fails.values()), (ctx, fails)
    # on the guard, not merely beyond it
    if k.guard == "F":
        assert t["F"] == (cc + 1 if k.claim == "decided" else cc) or k.name.startswith("c = n - 1"), (ctx, t)
    if k.guard == "G":
        assert t["G"] == (cc + 1 if k.claim == "decided" else cc), (ctx, t)
    if k.guard == "length":
        assert t["tmin"] == (fc.W if k.claim == "decided" else fc.W - 1), (ctx, t)
    if k.guard == "cap":
        assert m in ((fc.CAP - 1, fc.CAP) if k.claim == "decided" else (fc.CAP + 1, fc.CAP + 2)), (ctx, m)
    return got, m


def test_constants_are_the_headers():
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yacrd_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("sweep_filtered.h", "screen_reg.h", "finish_compact.h")}
    assert int(re.search(r"constexpr int kFilteredCap = (\d+);", text["sweep_filtered.h"]).group(1)) == fc.CAP
    assert int(re.search(r"#define YK_SCREEN_WINDOW (\d+)", text["screen_reg.h"]).group(1)) == fc.W
    assert "filtered_turn<%d, (int)kWaves, kTabWords>" % fc.NB in text["finish_compact.h"]
    assert fc.sh_of(fc.L20) == 16 and fc.sh_of(1000) == 5 and fc.sh_of(1024) == 6


@pytest.mark.parametrize("c", fc.COVS)
def test_every_case_is_what_it_says(c):
    names = set()
    for k in fc.cases(c):
        assert k.name not in names
        names.add(k.name)
        check_case(k, c)
    assert len(names) >= 30


def test_interval_counts_against_the_threshold():
    for c, k in fc.special_cases():
        check_case(k, c)
    assert {c for c, _ in fc.special_cases()} >= {65, 64, 0xFFFFFFFF}


def test_the_set_stands_on_both_sides_of_every_guard():
    """a condition of the set: for every guard a case the filter decides AND one it leaves, at every threshold where both exist
    (F = c and G = c need c >= 1; n <= c lives in special_cases)"""
    for c in fc.COVS:
        sides = {}
        for k in fc.cases(c):
            if k.guard:
                sides.setdefault(k.guard, set()).add(k.claim)
        for g in ("cap", "length"):
            assert sides[g] == {"decided", "left"}, (c, g)
        for g in ("F", "G"):
            assert sides[g] == ({"decided", "left"} if c >= 1 else {"decided"}), (c, g)
        ms = {m for _, m in (fc.filtered(k.iv, k.L, c) for k in fc.cases(c)) if m is not None}
        assert {127, 128, 129} <= ms, (c, sorted(ms))
        assert {len(k.iv) for k in fc.cases(c)} >= set(fc.SIZES)
    special = {(k.guard, k.defer) for _, k in fc.special_cases()}
    assert ("n", False) in special and ("F", True) in special
    # n > c decided: every decided case above; n <= c left: special_cases


@pytest.mark.parametrize("c", fc.COVS)
def test_block_and_run_cases_have_their_shape(c):
    by = {k.name: k for k in fc.cases(c)}

    def inner(k):  # the oracle's regions that touch neither end of the read
        return [r for r in oracle_regions(k.iv, k.L, c) if r[0] != 0 and r[1] != k.L]

    assert len(inner(by["two holes"])) == 2 and len(inner(by["three holes"])) == 3
    assert inner(by["abutting halves"]) in ([(fc.L20 // 2, fc.L20 // 2)], [])  # (a zero-length gap, if the reference reports one)
    assert inner(by["a gap of one position"]) == [(fc.L20 // 2, fc.L20 // 2 + 1)]
    same_lane = 0
    for k_front in range(4):
        k = by["two runs in one lane, %d in front" % k_front]
        assert inner(k) == [(200000, 300000), (300040, 300090), (300130, 400000)], k.name
        i1 = 40 + k_front + 1  # island 1's end among the sorted kept keys: A's ends, then s1, e1, s2, e2
        keys = sorted([e for s, e in k.iv if e < 300000 and e != fc.L20] + [300000, 300040, 300090, 300130])
        assert keys[i1] == 300040 and keys[i1 + 2] == 300130
        same_lane += (i1 // 4) == ((i1 + 2) // 4)  # (sweep_filtered.h: K = kFilteredCap / LANES = 4 sorted keys per lane)
    assert same_lane >= 2
    # the junction on a border: a start AT a multiple of 2^sh, every near end in the block in front
    k = by["junction on a block border"]
    sh = fc.sh_of(k.L)
    assert any(s == 8 << sh for s, e in k.iv) and {e >> sh for s, e in k.iv if abs(e - (8 << sh)) <= 64} == {7}
    # events behind T: the tail window lies across a block border
    k = by["events behind T"]
    t = fc.table(k.iv, k.L)
    span = t["pmax"] - t["pmin"]
    assert (span - fc.W) >> sh < span >> sh and t["pmin"] > 0 and t["pmax"] < k.L
    k = by["window pmin>0 pmax<len"]
    assert fc.table(k.iv, k.L)["pmin"] > 0 and fc.table(k.iv, k.L)["pmax"] < k.L
    assert fc.sh_of(by["short read n65"].L) == 5  # a block as wide as a window


def test_orderings_and_filler():
    for c in fc.COVS:
        o = dict(fc.orderings(c))
        assert len(o["decided"]) >= 25 and len(o["left"]) >= 5
        assert all(k.claim == "decided" for k in o["alternating"][0::2]) and all(k.claim == "left" for k in o["alternating"][1::2])
        assert {k.name for k in o["alternating"]} == {k.name for k in o["decided"]} | {k.name for k in o["left"]}
    marked = [(np.array(k.iv, np.uint32), k.L) for k in fc.cases(0)[:3]]
    off, iv, ln = fc.with_filler(marked, [0, 5, 9], 10)
    assert len(off) == 11 and int(off[-1]) == len(iv) and ln[5] == marked[1][1] and ln[4] == 1000
    assert np.array_equal(iv[int(off[9]):int(off[10])], marked[2][0]) and (np.diff(off.astype(np.int64))[[1, 2, 3]] == [2, 3, 1]).all()
    want = oracle.run(off, iv, ln.astype(np.uint64), 0, 0.4, n_threads=1)
    assert int(want[0][2]) - int(want[0][1]) == 0  # (filler: covered from end to end)
    assert formulation.bin_shift(1000, fc.NB) == 5
