"""The yardstick at large coordinates, and the conditions that keep tests/test_gpu_coordinates.py from going hollow.  CPU only.

The oracle is pinned on the reference's golden files, which are all at small coordinates.  src/stack.rs only compares positions
with each other, with 0 and with the length, so multiplying every start, every end and the length by k must multiply every
region by k: that proves the oracle's u32 handling up to 2^32 - 1 from its behaviour at small values.  The emulations of the
two GPU formulations (tests/formulation.py) must then equal the oracle there, and the regular one must decline a read exactly
when the event keys cannot hold it."""
import numpy as np
import pytest

import oracle
import coordinate_cases as cc
from cases import make_csr, make_read
from coordinate_cases import K, U32
from formulation import general_events, regular_events

FACTORS = (2, 2**20, None)  # None: the largest k that keeps every value of the read <= 2^32 - 1
COVERAGES = (0, 1, 4)


def _reads_of(mode, count=300):
    rng = np.random.default_rng(cc.ALL_MODES.index(mode) + 20)
    for it in range(count):
        n = int(rng.integers(0, 40)) if it % 4 else int(rng.integers(40, 300))
        L = int(rng.integers(1, 3000)) if it % 3 else int(rng.integers(1, 60))
        yield [tuple(int(x) for x in p) for p in make_read(rng, n, L, mode)], L


def _times(iv, k):
    return [(s * k, e * k) for s, e in iv]


def _declines(iv):
    """Whether the regular formulation must leave the read to the exact path: an end beyond the keys' range, a start beyond
    its end, or two zero-length intervals at one position > 0 (the cause formulation.regular_keys documents; it does not
    depend on the scale)."""
    zero = [s for s, e in iv if s == e and s != 0]
    return any(e > K or s > e for s, e in iv) or len(zero) != len(set(zero))


@pytest.mark.parametrize("mode", cc.ALL_MODES)
def test_oracle_and_formulations_scale(mode):
    """300 reads of the mode, c in (0, 1, 4), k in (2, 2^20, the largest that fits): the oracle's regions scale by k, and
    both emulations equal the oracle on the scaled read.  7 modes x 300 x 3 x 3 = 18 900 cases."""
    declined = kept = 0
    for iv, L in _reads_of(mode):
        top = max([L] + [e for _, e in iv] + [s for s, _ in iv])
        for cov in COVERAGES:
            base = oracle.compute_bad_part(iv, L, cov)
            for k in FACTORS:
                k = U32 // top if k is None else k
                assert k * top <= U32
                big = _times(iv, k)
                want = oracle.compute_bad_part(big, L * k, cov)
                assert want == _times(base, k), (mode, iv, L, cov, k)
                assert general_events(big, L * k, cov) == want, (mode, iv, L, cov, k)
                reg = regular_events(big, L * k, cov)
                if len(iv):
                    assert (reg is None) == _declines(big), (mode, iv, L, cov, k)
                if reg is None:
                    declined += 1
                else:
                    kept += 1
                    assert reg == want, (mode, iv, L, cov, k)
    assert declined > 0 and kept > 0  # both sides of the keys' range are in it


EDGE_ENDS = (0x3FFFFFFD, 0x3FFFFFFE, 0x3FFFFFFF, 0x40000000)


@pytest.mark.parametrize("mode", cc.ALL_MODES)
def test_formulations_on_the_edge_of_the_key_range(mode):
    """Scaled reads with one interval's end, one interval's two positions, or the length put on 0x3FFFFFFD .. 0x40000000:
    the emulations equal the oracle, and the regular one declines from 0x3FFFFFFF on."""
    seen = set()
    for it, (iv, L) in enumerate(_reads_of(mode, 80)):
        if not iv:
            continue
        top = max([L] + [e for _, e in iv] + [s for s, _ in iv])
        k = (2**30 - 64) // top  # everything below the edge, the largest value next to it
        big, j = _times(iv, k), it % len(iv)
        for E in EDGE_ENDS:
            for what in range(4):
                ed, Lk = list(big), L * k
                if what == 0:
                    ed[j] = (min(ed[j][0], E), E)      # an end on the edge
                elif what == 1:
                    ed[j] = (E, E)                     # a zero-length interval there
                elif what == 2:
                    ed[j] = (min(ed[j][0], E), E)
                    Lk = E                             # ... and the read ends there
                else:
                    Lk = E                             # only the length
                for cov in COVERAGES:
                    want = oracle.compute_bad_part(ed, Lk, cov)
                    assert general_events(ed, Lk, cov) == want, (mode, ed, Lk, cov)
                    reg = regular_events(ed, Lk, cov)
                    assert (reg is None) == _declines(ed), (mode, ed, Lk, cov)
                    assert reg is None or reg == want, (mode, ed, Lk, cov)
                    if what < 3:
                        seen.add((E, reg is None))
    for E in EDGE_ENDS:  # an end up to kMaxKeyPos is kept (unless something else declines the read), a larger one never
        assert (E, True) in seen or E <= K
        assert ((E, False) in seen) == (E <= K), (E, seen)


def test_oracle_read_type_scales():
    """oracle.run's read_type on the scaled batch equals the unscaled one: for region lists the oracle produced the u32 sum
    of the regions' lengths does not wrap as long as no region ends before it begins, and a correctly rounded f64 quotient is
    unchanged when numerator and denominator are scaled alike."""
    seen = set()
    for seed, mode_block in ((1, 1), (2, 3)):
        rng = np.random.default_rng(seed)
        sizes = np.concatenate([np.arange(0, 30), rng.integers(1, 300, size=600)])
        csr = make_csr(seed, sizes, cc.ALL_MODES, len_lo=1, len_hi=3000, mode_block=mode_block)
        for k in (2, 2**20, U32 // cc.max_value(csr)):
            big = cc.scaled(csr, k)
            for cov in COVERAGES:
                for nc in (0.0, 0.1, 0.4, 0.8, 1.0):
                    bo, br, rt = oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), cov, nc)
                    bo2, br2, rt2 = oracle.run(big[0], big[1], big[2].astype(np.uint64), cov, nc)
                    assert np.array_equal(bo, bo2) and np.array_equal(br.astype(np.uint64) * np.uint64(k), br2)
                    # (a region the oracle reports may end before it begins — a read with start > end intervals —, and then
                    # the u32 sum wraps and the type need not survive the scaling: those reads are left out)
                    width = br2[:, 1].astype(np.int64) - br2[:, 0]
                    owner = np.repeat(np.arange(len(rt)), np.diff(bo2.astype(np.int64)))
                    total, wraps = np.zeros(len(rt), np.int64), np.zeros(len(rt), bool)
                    np.add.at(total, owner, width)
                    wraps[owner[width < 0]] = True
                    wraps |= total > U32
                    assert int(wraps.sum()) * 2 < len(rt)
                    assert np.array_equal(rt[~wraps], rt2[~wraps]), (seed, k, cov, nc, np.nonzero((rt != rt2) & ~wraps)[0][:5])
                    seen.update(rt[~wraps].tolist())
                    for r in np.nonzero(~wraps)[0][::37]:  # and type_of_read alone on the oracle's own lists
                        regs = br2[int(bo2[r]):int(bo2[r + 1])].tolist()
                        assert oracle.type_of_read(int(big[2][r]), regs, nc) == int(rt[r])
    assert seen == {0, 1, 2}


# ---- the GPU file's batches: conditions asserted here, where they run without a GPU ----------------------------------------
def _profile(csr, cov=4):
    """-> (some region begins beyond K, some region ends beyond K, the region counts that occur, the types that occur)"""
    offsets, intervals, lengths = csr
    assert intervals.dtype == np.uint32 and lengths.dtype == np.uint32 and offsets.dtype == np.uint64
    assert len(offsets) == len(lengths) + 1 and int(offsets[-1]) == len(intervals)
    bo, br, rt = oracle.run(offsets, intervals, lengths.astype(np.uint64), cov, 0.4, n_threads=4)
    counts = set(np.unique(np.diff(bo.astype(np.int64))).tolist())
    return bool((br[:, 0] > K).any()), bool((br[:, 1] > K).any()), counts, set(np.unique(rt).tolist())


@pytest.mark.parametrize("which", cc.SCREEN_BATCHES)
def test_screen_batches_reach_beyond_the_key_range(which):
    csr = cc.screen_batch(which)
    begin, end, counts, types = _profile(csr)
    assert begin and end, "no region begins / ends beyond kMaxKeyPos"
    assert {2, 3} <= counts and types == {0, 1, 2}, (counts, types)
    assert set(np.unique(csr[2]).tolist()) == set({"register": cc.SWEEP_LENGTHS, "workgroup": cc.WORKGROUP_LENGTHS,
                                                   "device_wide": cc.BIG_LENGTHS}[which])
    small = cc.sub_batch(csr, csr[2] <= K)  # the sub-batch the GPU tests take the screens' counters on
    assert 0 < len(small[2]) < len(csr[2]) and int(small[2].max()) == K and int(small[0][-1]) == len(small[1])


def test_screen_batches_together_hold_every_count_and_type():
    counts = set()
    for which in cc.SCREEN_BATCHES:
        counts |= _profile(cc.screen_batch(which))[2]
    assert {0, 1, 2, 3} <= counts, counts


@pytest.mark.parametrize("size", cc.CLASS_SIZES)
def test_class_batches_reach_beyond_the_key_range(size):
    """Each class's batches: the four goals' largest lengths land where they should, k = 1 holds nothing beyond K, and the
    scaled batches together hold regions that begin and that end beyond K."""
    begin = end = False
    counts, types = set(), set()
    for goal, (top, target) in cc.GOALS.items():
        csr, k = cc.class_batch(size, goal)
        n = np.diff(csr[0].astype(np.int64))
        assert (n == size).all() and int(csr[2].min()) >= 500 and int(csr[2].max()) == top <= 4000
        big = cc.scaled(csr, k)
        if target is not None:
            assert int(big[2].max()) == target
        else:
            assert cc.max_value(big) <= U32 < cc.max_value(csr) * (k + 1) and int(big[2].max()) > U32 - 4000
        b, e, c, t = _profile(big)
        assert (b and e) or target in (K, K + 1)  # (the two goals on the edge leave at most one position beyond it)
        begin, end, counts, types = begin or b, end or e, counts | c, types | t
        b1, e1, c1, t1 = _profile(csr)
        assert not b1 and not e1 and c1 == c and t1 == t
    assert begin and end, "no region begins / ends beyond kMaxKeyPos"


def test_class_batches_together_hold_every_count_and_type():
    counts, types = set(), set()
    for size in cc.CLASS_SIZES:
        _, _, c, t = _profile(cc.class_batch(size, "2^31")[0])
        counts, types = counts | c, types | t
    assert {0, 1, 2, 3} <= counts and types == {0, 1, 2}, (counts, types)


@pytest.mark.parametrize("n", cc.EDGE_SIZES)
def test_edge_batches(n):
    csr = cc.edge_batch(n)
    offsets, intervals, lengths = csr
    assert (np.diff(offsets.astype(np.int64)) == n).all()
    G = cc.group_size(n)
    per_length = len(cc.EDGE_ENDS) * len(cc.EDGE_SHAPES) * G * G
    assert len(lengths) == len(cc.EDGE_LENGTHS) * per_length + 4 * G * G
    iv = intervals.reshape(len(lengths), n, 2)
    plain = (iv[:, :, 0] < iv[:, :, 1]).all(axis=1) & (iv[:, :, 1] <= lengths[:, None]).all(axis=1)
    edited = 0
    for g in range(0, len(cc.EDGE_LENGTHS) * per_length, G):  # one edited read per group, in every slot in turn
        slot = (g // G) % G
        for j in range(G):
            r = g + j
            if j == slot:
                assert int(lengths[r]) in cc.EDGE_LENGTHS
                edited += 1
            else:
                assert plain[r] and int(lengths[r]) in cc.NEIGHBOUR_LENGTHS
    assert edited == len(cc.EDGE_LENGTHS) * len(cc.EDGE_ENDS) * len(cc.EDGE_SHAPES) * G
    for E in cc.EDGE_ENDS:  # every edit is there
        for shape in cc.EDGE_SHAPES:
            s, e = shape(E)
            assert ((intervals[:, 0] == s) & (intervals[:, 1] == e)).any()
    if G > 1:
        below = lengths[plain & np.isin(lengths, cc.NEIGHBOUR_LENGTHS)]
        assert (below < K).any() and (below > K).any()
    tail = slice(len(cc.EDGE_LENGTHS) * per_length, None)
    low = plain[tail] & (iv[tail, :, 1].max(axis=1) <= 10**6) & (lengths[tail] > K)
    high = plain[tail] & (iv[tail, :, 0].min(axis=1) >= K - 10**6) & (lengths[tail] == K)
    assert int(low.sum()) >= 3 * G and int(high.sum()) >= G
    begin, end, counts, types = _profile(csr)
    assert begin and end


def test_edge_batches_together_hold_every_count_and_type():
    counts, types = set(), set()
    for n in cc.EDGE_SIZES:
        _, _, c, t = _profile(cc.edge_batch(n))
        counts, types = counts | c, types | t
    assert {0, 1, 2, 3} <= counts and types == {0, 1, 2}, (counts, types)


@pytest.mark.parametrize("m4", [False, True])
def test_edge_text(m4):
    text = cc.edge_text(m4)
    reads = (oracle.parse_m4 if m4 else oracle.parse_paf)(text)
    names, offsets, intervals, lengths = oracle.to_csr(reads)
    assert 24 <= text.count("\n") <= 48 and sorted(lengths.tolist()) == [K, K + 1, U32] and int(offsets[-1]) == 2 * text.count("\n")
    assert int(intervals.max()) == U32  # the largest value the parsers accept
    for E in cc.EDGE_ENDS:
        for shape in cc.EDGE_SHAPES:
            s, e = shape(E)
            assert ((intervals[:, 0] == s) & (intervals[:, 1] == e)).any()
