"""Reads of more than 16 384 intervals (class CLS_GENERAL, "BIG") made for ONE tier of the cascade each:
  tier 0  csrc/screen_big.h       the device-wide healthy-read screen
  tier 1  csrc/sweep_big_trim.h   the trimming filter, what is left swept in LDS (at most kBtCap = 16 384 keys)
  tier 2  csrc/sweep_big.h        the segmented sort and its chunked sweep
  tier 3  csrc/sweep_general.h    the exact kernel
What tests/test_big_cases.py (CPU: the generators do what they say, against tests/formulation.py's emulations) and
tests/test_gpu_big_tiers.py (GPU: the oracle's bytes and Engine.big_routes()) share.  Generators only, vectorised numpy: nothing
here runs the oracle or the engine.  Every read is seeded.

A shape is a function of (rng, n, L, c) that returns n intervals with start < end <= L unless its text says otherwise;
`routes(shape, n, L, c, flags)` is its CLAIM: what Engine.big_routes() adds up to for that one read.  The claims hold for the
coverages of COVS alone (c <= 4, or c >= n - 1: nothing is ever deep then): that is asserted, not assumed."""
import functools

import numpy as np

N_SMALL, N_CHUNKED = 16385, 20000  # the smallest BIG read (a last chunk of ONE interval on the 4096-interval grids), and another
SIZES = (N_SMALL, N_CHUNKED)
K_BT_CAP = 16384  # kBtCap
SHORT_LENGTHS = (1, 2, 3, 100, 1023, 1024, 1025, 1026, 1027, 1055, 1056, 2047, 2048, 2049, 3071, 3072, 3073, 5000, 65536,
                 2**19 - 1, 2**19, 2**19 + 1)
F_NO_PREFILTER, F_FORCE_GENERAL = 256, 1  # include/yacrd_engine_debug.h


def covs(n):
    return (0, 4, n - 1, n, 0xFFFFFFFF)


def _u(rng, lo, hi, size):
    """uniform integers in [lo, hi], hi raised to lo where the read is too short for the range"""
    lo = int(lo)
    return rng.integers(lo, max(int(hi), lo) + 1, size=size, dtype=np.int64)


def _out(s, e):
    return np.stack([s, e], axis=1).astype(np.uint32)


def pile(rng, n, L, c=0):
    """A third dovetails from within 16 positions of 0 (ending in the second half), a third to within 16 positions of L (starting
    in the first half), the rest span the middle (L/4 .. 3L/4, across L/2).  One interval starts at 0 and one ends at L, so the
    covered span is L.  More than n // 3 intervals are open everywhere between position 16 and L - 16: the device-wide screen
    decides it whenever L >= 1024 (its span of 2 * 512) and n // 3 > c.  Degrades to the few intervals a read of L <= 3 has."""
    w, h = min(16, (L - 1) // 4), L // 2
    a, b = n // 3, n // 3
    m = n - a - b
    ls, le = _u(rng, 0, w, a), _u(rng, max(h, 1), L - w - 1, a)
    rs, re = _u(rng, min(w + 1, max(h - 1, 0)), max(h - 1, 0), b), _u(rng, L - w, L, b)
    ms, me = _u(rng, L // 4, h - 1, m), np.minimum(_u(rng, h + 1, 3 * L // 4, m), L)
    ls[0], re[0] = 0, L
    s, e = np.concatenate([ls, rs, ms]), np.concatenate([le, re, me])
    assert (s < e).all() and e.max() <= L
    return _out(s, e)


def holed(rng, n, L, c=0):
    """Two piles that do not meet: one from within 16 positions of 0 to L/5 .. 2L/5, one from 3L/5 .. 4L/5 to within 16 positions of
    L, so nothing covers the middle fifth.  The screen refuses it (the second pile's first starts are shallow); of each pile
    the trimming filter keeps the outermost events: a few dozen to a few hundred keys."""
    w = min(16, L // 8)
    a = n // 2
    b = n - a
    s = np.concatenate([_u(rng, 0, w, a), _u(rng, 3 * L // 5 + 1, 4 * L // 5, b)])
    e = np.concatenate([_u(rng, L // 5, 2 * L // 5 - 1, a), _u(rng, L - w, L, b)])
    s[0], e[-1] = 0, L
    assert (s < e).all() and e.max() <= L and w < L // 5
    return _out(s, e)


def window(rng, n, L, c=0):
    """Every interval inside [L/3, 2L/3]: a pile of length L // 3 moved up by L // 3, so the covered span is L // 3 (1023 at
    L = 3071, 1024 at 3072)."""
    return (pile(rng, n, L // 3, c).astype(np.int64) + L // 3).astype(np.uint32)


def comb_depth(n, L):
    return -(-n // L)


def comb(rng, n, L, c=0):
    """n intervals of ONE position, (s, s + 1), laid evenly over 0 .. L - 1: disjoint (abutting) where L >= n, else
    comb_depth(n, L) = ceil(n / L) deep at most.  The screen refuses it at any c (no start is entered at a depth beyond 0 once
    its bin's ends are taken off).  The trimming filter keeps all 2 n keys while that depth is at most c + 1: a position then
    holds at most c + 1 starts, each among the first c + 1 of its one-position bin, and no interval spans a wider bin."""
    s = (np.arange(n, dtype=np.int64) * L) // n
    s = s[rng.permutation(n)]
    return _out(s, s + 1)


def comb_plus_pile(rng, n, L, c=0, k=64):
    """A pile of n - k intervals over the first half (length L // 2) and exactly k disjoint one-position intervals in the second,
    at L/2 + 2, L/2 + 4, ...: two keys each survive the trimming filter, of the pile a few hundred do.  The pile is drawn first:
    with one seed, n - k fixed and k growing, only the comb grows (the knob for the kBtCap edge)."""
    assert L // 2 + 2 * k + 3 <= L - 600 and n > k
    p = pile(rng, n - k, L // 2, c)
    s = L // 2 + 2 + 2 * np.arange(k, dtype=np.int64)
    return np.concatenate([p, _out(s, s + 1)])


def beyond(rng, n, L, c=0):
    """pile with one end at L + 1 (BT_PLAIN_NO: neither the screen nor the trimming filter take it; the sort does)"""
    iv = pile(rng, n, L, c)
    iv[n // 2, 1] = L + 1
    return iv


def reversed_(rng, n, L, c=0):
    """holed with one interval (3, 2) (BT_BAD: start > end, the exact kernel's)"""
    iv = holed(rng, n, L, c)
    iv[n // 2] = (3, 2)
    return iv


ZL_P = 9000  # the position of zl_pair_at's two zero-length intervals
ZL_T = (5, 31, 32, 8191, 8192)  # inside a thread's run of kBigKT = 32 keys, across a thread border, across a chunk border (kBigC = 8192)


def zl_pair_at(rng, n, L, c=0, t=5):
    """Exactly t keys sort in front of two zero-length intervals at one position p = ZL_P: t plain starts at 0 .. t - 1 (their
    ends at p + 1 + j), and every other start — a comb of one-position intervals, two positions apart — lies above all of them.
    The comb's 2 (n - t - 2) keys are more than kBtCap, so the trimming filter cannot thin the read and it reaches the sort
    at default flags; pass A must send it to the exact kernel."""
    r = n - t - 2
    assert 0 < t < ZL_P and 2 * r > K_BT_CAP and ZL_P + t + 10 + 2 * r < L
    j = np.arange(t, dtype=np.int64)
    cs = ZL_P + t + 10 + 2 * np.arange(r, dtype=np.int64)
    s = np.concatenate([j, [ZL_P, ZL_P], cs])
    e = np.concatenate([ZL_P + 1 + j, [ZL_P, ZL_P], cs + 1])
    return _out(s, e)[rng.permutation(n)]


SHAPES = {"pile": pile, "holed": holed, "window": window, "comb": comb, "comb_plus_pile": comb_plus_pile, "beyond": beyond,
          "reversed": reversed_}


def tier(shape, n, L, c):
    """The tier that decides the read at default flags, or None where the shape has no room at this length (or makes no claim at
    this coverage).  The rules are read off the kernels; tests/test_big_cases.py holds every one against the emulations."""
    assert c <= 4 or c >= n - 1
    nothing_deep = c >= n - 1  # (then the screen refuses — it needs c + 1 starts in 512 positions — and all 2 n keys survive)
    if shape in ("pile", "beyond"):
        if shape == "beyond":
            return 2
        if nothing_deep:
            return 2
        # L <= 3: every start lies at position 0, entered at depth 0: all kept
        return 0 if L >= 1024 else 1 if L >= 100 else 2
    if shape == "window":
        if L < 100:
            return None
        return 2 if nothing_deep else 0 if L // 3 >= 1024 else 1
    if shape == "holed":
        return None if L < 100 else 2 if nothing_deep else 1
    if shape == "reversed":
        return None if L < 100 else 3
    if shape == "comb":
        d = comb_depth(n, L)
        return 2 if (nothing_deep or d <= c + 1) else None
    if shape == "comb_plus_pile":
        return None if L < 2048 else 2 if nothing_deep else 1
    raise ValueError(shape)


def routes(shape, n, L, c, flags=0):
    """Engine.big_routes() of a batch that holds this one BIG read"""
    t = 2 if shape == "zl_pair_at" else tier(shape, n, L, c)
    assert t is not None
    if flags & F_FORCE_GENERAL:
        return (0, 0, 0, 1)
    if flags & F_NO_PREFILTER:  # the sort takes everything; a reversed interval is found by its fill
        return (0, 0, 1, 1 if shape in ("reversed", "zl_pair_at") else 0)
    if shape == "zl_pair_at":
        return (0, 0, 1, 1)
    return tuple(1 if i == t else 0 for i in range(4))


def fits(n, c):
    """[(shape, L)] of the matrix at this size and coverage: every shape at every length of SHORT_LENGTHS where it has room
    (and makes a claim: `comb` is left out where it is more than c + 1 deep)"""
    return [(shape, L) for L in SHORT_LENGTHS for shape in SHAPES if tier(shape, n, L, c) is not None]


def _check_matrix():
    for n in SIZES:
        for c in covs(n):
            here = fits(n, c)
            for shape in SHAPES:
                if not (shape == "comb" and c == 0):  # (at most one deep only where L >= n: four lengths)
                    assert sum(1 for s, _ in here if s == shape) >= 5, (shape, n, c)
            for L in SHORT_LENGTHS:
                assert ("pile", L) in here or ("comb", L) in here, (L, n, c)


_check_matrix()


def seed_of(shape, n, L, c):
    return [4100, sorted(SHAPES).index(shape), n, L, min(c, 2**31)]


def matrix(ci):
    """The matrix's batch for the ci-th coverage of COVS: every shape at every length it fits, in a seeded shuffle.  At c = 0, 4
    and 0xFFFFFFFF the reads alternate between the two sizes; c = n - 1 is taken at n = N_SMALL and c = n at n = N_CHUNKED (one
    coverage per batch: every read of it must have that n).  Returns (c, [(shape, n, L, intervals)])."""
    sizes = {2: (N_SMALL,), 3: (N_CHUNKED,)}.get(ci, SIZES)
    c = covs(sizes[0])[ci]
    reads = []
    for i, (shape, L) in enumerate(x for x in fits(sizes[0], c) if x in fits(sizes[-1], c)):
        n = sizes[i % len(sizes)]
        iv = SHAPES[shape](np.random.default_rng(seed_of(shape, n, L, c)), n, L, c)
        assert iv.shape == (n, 2) and iv.dtype == np.uint32
        reads.append((shape, n, L, iv))
    order = np.random.default_rng([4101, ci]).permutation(len(reads))
    return c, [reads[i] for i in order]


def csr_of(reads):
    """[(intervals u32[n, 2], L)] -> offsets u64, intervals u32[I, 2], lengths u32"""
    offsets = np.zeros(len(reads) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(iv) for iv, _ in reads])
    intervals = np.concatenate([iv for iv, _ in reads]) if reads else np.zeros((0, 2), np.uint32)
    return offsets, np.ascontiguousarray(intervals, dtype=np.uint32), np.array([L for _, L in reads], dtype=np.uint32)


def sorted_keys(iv):
    """formulation.regular_keys' sorted keys (pos << 2 | class: 0 end, 1 / 2 zero-length start / end, 3 start), vectorised"""
    s, e = iv[:, 0].astype(np.uint64), iv[:, 1].astype(np.uint64)
    z = np.where(s == e, 2, 0).astype(np.uint64)
    k = np.concatenate([((s << np.uint64(2)) | np.uint64(3)) - z, (e << np.uint64(2)) + z])
    k.sort()
    return k


# ---- the kBtCap edge: bt_plan_kernel's `fits` (m_new <= kBtCap) ------------------------------------------------------------------
CAP_L, CAP_PILE = 65536, N_SMALL


def cap_read(c, k):
    """comb_plus_pile(k) on CAP_L with a pile of CAP_PILE intervals, the same pile for every k"""
    return comb_plus_pile(np.random.default_rng([4103, c]), CAP_PILE + k, CAP_L, c, k)


def trim_key_count(iv, L, c):
    """keys the trimming filter keeps of a plain read: formulation.trim_keys at the device-wide geometry (1024 coarse bins, fine
    zones of 512).  Read against bt_plan_kernel and TrimGeo<1024, 512> it is the kernel's m_new: the same fine zones (none below
    L = 1026, the right one from L - 511 on), the same coarse shift, the same quotas per bin, and a stand-in key for each unit of
    depth dropped in front of a bin that keeps something.  (The emulation lets an EMPTY coarse bin behind position L - 512 keep
    "something" where the kernel has no such bin; it gives that bin the stand-ins the kernel gives the next one, the count is the
    same.)  Always even: the kept keys are a balanced set of starts and ends."""
    import formulation
    return len(formulation.trim_keys([tuple(x) for x in iv.tolist()], L, c, 1024, 512))


@functools.lru_cache(maxsize=None)
def cap_k(c):
    """the k at which cap_read(c, k) keeps exactly kBtCap keys (two more per further interval of the comb)"""
    k0 = 7000
    k = k0 + (K_BT_CAP - trim_key_count(cap_read(c, k0), CAP_L, c)) // 2
    assert 0 < k < 8000
    return k


# ---- the read of more than 2^20 intervals: big_scan_kernel's second trip over a read's chunks ------------------------------
# (c = 2, not 1: the depth entering a key has the parity of the key's index, so in front of an even index it is 0 or >= 2)
HUGE_N, HUGE_L, HUGE_C = 1_100_000, 3_000_000, 2
HUGE_KEY = 256 * 8192  # the first key of the 257th chunk: kBigT chunks of kBigC keys lie in front of it


@functools.lru_cache(maxsize=None)
def huge_sparse():
    """About HUGE_N intervals of 1 .. 3 positions on HUGE_L, low coverage with holes everywhere (cases.make_read's "sparse", laid
    out uniformly): 2.2 M keys, P = 2^22, 512 chunks.  The few intervals that end first are dropped until, at c = HUGE_C, the key
    at index HUGE_KEY is entered at a depth of 1 .. c and left at <= c, with its neighbours at other positions: then it lies
    strictly inside a region (the depth scan's carry decides that), and regions close on both sides of it (the closing scan's
    carry places them, the max scan's carries shape the ones behind it)."""
    rng = np.random.default_rng(4105)
    s = rng.integers(0, HUGE_L - 4, size=HUGE_N, dtype=np.int64)
    e = s + rng.integers(1, 4, size=HUGE_N, dtype=np.int64)
    k = sorted_keys(_out(s, e))
    step = np.where(k & np.uint64(1), 1, -1).astype(np.int64)
    d_in = np.cumsum(step) - step
    pos = (k >> np.uint64(2)).astype(np.int64)
    i = np.arange(HUGE_KEY, HUGE_KEY + 4096, 2)
    ok = (d_in[i] >= 1) & (d_in[i] <= HUGE_C) & (d_in[i] + step[i] <= HUGE_C) & (pos[i - 1] < pos[i]) & (pos[i] < pos[i + 1])
    m = int(i[np.nonzero(ok)[0][0]] - HUGE_KEY) // 2  # intervals to drop in front of the key: two keys each
    keep = np.argsort(e, kind="stable")[m:]
    assert m == 0 or e[np.argsort(e, kind="stable")[m - 1]] < pos[HUGE_KEY] - 8
    keep.sort()
    return _out(s[keep], e[keep])
