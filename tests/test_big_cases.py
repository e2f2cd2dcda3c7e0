"""tests/big_cases.py's reads do what they say (no GPU): every claim of a tier is held against the CPU emulations of
tests/formulation.py at the device-wide instantiations (1024 coarse bins, windows / fine zones of 512) and against the oracle."""
import numpy as np
import pytest

import big_cases as bc
import formulation
import oracle

PLAIN_SHAPES = ("pile", "holed", "window", "comb", "comb_plus_pile")


def as_list(iv):
    return [tuple(x) for x in iv.tolist()]


def oracle_regions(iv, L, c):
    bo, br, _ = oracle.run(np.array([0, len(iv)], np.uint64), iv, np.array([L], np.uint64), c, 0.4, n_threads=1)
    return [tuple(x) for x in br.tolist()]


def test_module_shape():
    assert len(bc.SHORT_LENGTHS) == 22 and set(bc.SHAPES) == {"pile", "holed", "window", "comb", "comb_plus_pile", "beyond", "reversed"}
    for n in bc.SIZES:
        assert bc.covs(n) == (0, 4, n - 1, n, 0xFFFFFFFF)
    for ci in range(5):
        c, reads = bc.matrix(ci)
        tiers = {bc.tier(shape, n, L, c) for shape, n, L, _ in reads}
        assert tiers == ({0, 1, 2, 3} if c <= 4 else {2, 3}), (c, tiers)
        for shape, n, L, iv in reads:
            if shape == "beyond":
                assert (iv[:, 0] < iv[:, 1]).all() and int(iv[:, 1].max()) == L + 1
            elif shape == "reversed":
                assert int((iv[:, 0] > iv[:, 1]).sum()) == 1 and (3, 2) in as_list(iv[iv[:, 0] > iv[:, 1]])
            else:
                assert (iv[:, 0] < iv[:, 1]).all() and int(iv[:, 1].max()) <= L, (shape, L)
            if shape == "holed":
                assert not ((iv[:, 0] < 3 * L // 5) & (iv[:, 1] > 2 * L // 5)).any()
            if shape == "window":
                assert int(iv[:, 0].min()) == L // 3 and int(iv[:, 1].max()) == 2 * (L // 3)


@pytest.mark.parametrize("ci", range(5))
def test_the_screen_emulation_takes_tier_0_and_refuses_the_rest(ci):
    c, reads = bc.matrix(ci)
    took = 0
    for shape, n, L, iv in reads:
        t = bc.tier(shape, n, L, c)
        got = formulation.unified_screen_regions(as_list(iv), L, c, 1024, 512)
        if t == 0:
            assert got is not None, (shape, n, L, c)
            assert got == oracle_regions(iv, L, c), (shape, n, L, c)
            took += 1
        else:
            assert got is None, (shape, n, L, c, t)
    assert (took >= 10) == (c <= 4)


@pytest.mark.parametrize("ci", range(5))
def test_the_trim_emulation_thins_tier_1_and_not_tier_2(ci):
    """plain reads the screen refused: the filter's key count is at most kBtCap exactly for tier 1.  (At the three coverages
    beyond n - 2 nothing is deep and all 2 n keys survive; one length in three is enough there.)"""
    c, reads = bc.matrix(ci)
    seen = {1: 0, 2: 0}
    for i, (shape, n, L, iv) in enumerate(reads):
        t = bc.tier(shape, n, L, c)
        if shape not in PLAIN_SHAPES or t == 0 or (c > 4 and i % 3):
            continue
        m = bc.trim_key_count(iv, L, c)
        assert (m <= bc.K_BT_CAP) == (t == 1), (shape, n, L, c, m)
        assert c <= 4 or m == 2 * n
        assert m > 0 and m % 2 == 0
        seen[t] += 1
    assert seen[2] >= 4 and (seen[1] >= 20) == (c <= 4), seen


def test_the_comb_one_deeper_than_c_keeps_every_key():
    """tests/test_gpu_big_tiers.py's 1100-read batch has a comb of 20 481 intervals on 5000 positions at c = 4: five deep"""
    n, L, c = 20481, 5000, 4
    assert bc.comb_depth(n, L) == c + 1 and bc.tier("comb", n, L, c) == 2
    iv = bc.comb(np.random.default_rng(7), n, L, c)
    assert bc.trim_key_count(iv, L, c) == 2 * n
    assert formulation.unified_screen_regions(as_list(iv), L, c, 1024, 512) is None


@pytest.mark.parametrize("c", (0, 4))
def test_the_cap_edge_in_keys(c):
    """cap_k(c) intervals in the comb: exactly kBtCap keys, the last read that fits; one more: two keys more (a kept set of keys
    is balanced, so no plain read keeps 16 385)"""
    k = bc.cap_k(c)
    for kk, want in ((k, bc.K_BT_CAP), (k + 1, bc.K_BT_CAP + 2)):
        iv = bc.cap_read(c, kk)
        assert len(iv) == bc.CAP_PILE + kk > 16384
        assert bc.trim_key_count(iv, bc.CAP_L, c) == want
        assert formulation.unified_screen_regions(as_list(iv), bc.CAP_L, c, 1024, 512) is None


def test_the_read_of_2_to_the_20_intervals():
    iv = bc.huge_sparse()
    L, c, K = bc.HUGE_L, bc.HUGE_C, bc.HUGE_KEY
    assert 2**20 < len(iv) <= bc.HUGE_N
    keys = formulation.regular_keys(as_list(iv))
    assert keys is not None and 2**21 < len(keys) <= 2**22 and keys == bc.sorted_keys(iv).tolist()
    assert K == 256 * 8192
    depth = sum(1 if k & 1 else -1 for k in keys[:K])
    assert 1 <= depth <= c
    p = keys[K] >> 2
    regions = oracle_regions(iv, L, c)
    assert formulation.sweep_keys(keys, L, c) == regions
    assert any(b < p < e for b, e in regions)            # one opens in front of that key and closes behind it
    assert sum(1 for b, e in regions if e < p) > 1000 and sum(1 for b, e in regions if b > p) > 1000


@pytest.mark.parametrize("t", bc.ZL_T)
def test_zl_pair_at(t):
    n, L = bc.N_CHUNKED, bc.CAP_L
    iv = bc.zl_pair_at(np.random.default_rng([4104, t]), n, L, 4, t)
    assert len(iv) == n and int(iv[:, 1].max()) <= L
    assert int((iv[:, 0] == iv[:, 1]).sum()) == 2
    keys = bc.sorted_keys(iv).tolist()
    pair = (bc.ZL_P << 2) | 1
    assert keys[t] == keys[t + 1] == pair and keys.count(pair) == 2 and keys[t - 1] < pair
    assert formulation.regular_keys(as_list(iv)) is None  # the exact path's
    assert bc.routes("zl_pair_at", n, L, 4) == (0, 0, 1, 1)
