"""Reads of the classes R16 / H16 (65 .. 256 intervals) made for the follow-on step's LONG-BATCH form: the reads
the healthy-read screen defers are listed (csrc/finish_compact.h: mark_list_kernel), dealt out and taken two per wavefront through
the filtered exact sweep (csrc/sweep_filtered.h via filtered_turn<32>); what the filter leaves is sorted whole.  Every case sits on
one side of one of the filter's guards and SAYS which: `claim` is "decided" (the filter writes the read's regions) or "left" (the
read stays marked and is sorted whole), `guard` names the guard, `defer` says whether the screen defers the read at all.
What tests/test_follow_on_cases.py (CPU: the claims against tests/formulation.py's emulations and the oracle) and
tests/test_gpu_follow_on.py (GPU: the oracle's bytes, timing()["deferred_reads"] and debug_counters()["deferred_sorted"]) share.
Generators only: nothing here runs the oracle or the engine.  Every read is seeded."""
import collections
import functools

import numpy as np

import formulation

NB = 32    # filtered_turn<32>: LANES coarse blocks per read (csrc/finish_compact.h; sweep_filtered.h: NB = LANES)
W = 32     # kScreenWindow (csrc/screen_reg.h)
CAP = 128  # kFilteredCap (csrc/sweep_filtered.h)
COVS = (0, 1, 3, 4, 9)
K_MAX_KEY_POS = 2**30 - 2  # kMaxKeyPos (csrc/device_common.h), as formulation.py states it: length >= 2**30 - 1 is not taken
SIZES = (65, 128, 129, 255, 256)
L20 = 2**20
# include/yacrd_engine_debug.h
F_COUNT_PREFILTERED, F_ALWAYS_DEFER, F_SCREEN_ITEMS_2, F_SCREEN_DIRECT = 512, 8192, 524288, 8388608
GUARDS = ("n", "F", "G", "length", "cap")

Case = collections.namedtuple("Case", "name iv L claim guard defer m")


def sh_of(L):
    """the coarse blocks' shift: formulation.bin_shift, but blocks of at least W positions (sweep_filtered.h: sh)"""
    sh = formulation.bin_shift(L, NB)
    while (1 << sh) < W:
        sh += 1
    return sh


def table(iv, L):
    """what the guards look at: n, F (starts within W positions of the smallest start), G (ends within W positions of the largest
    end), the shortest interval"""
    pmin, pmax = min(s for s, e in iv), max(e for s, e in iv)
    return {"n": len(iv), "F": sum(1 for s, e in iv if s - pmin < W), "G": sum(1 for s, e in iv if pmax - e < W),
            "tmin": min(e - s for s, e in iv), "pmin": pmin, "pmax": pmax}


def filtered(iv, L, c):
    """(regions or None, m or None): the filtered sweep's emulation at the kernel's constants"""
    stats = []
    got = formulation.filtered_sweep_regions(list(iv), L, min(c, 0x3FFFFFFF), NB, W, CAP, stats)
    return got, (stats[0] if stats else None)


def screen_defers(iv, L, c):
    """Whether the long launch's screen (csrc/screen_reg.h: screen_reads, the two-items build: no second looks) marks the read
    for the follow-on step.  Its verdict is formulation.slid_window_screen_regions with no slide (= window_screen_regions on
    blocks counted from the smallest start, as the kernel counts them) at the read's own table — 16 coarse blocks for a read of
    R16 (at most 128 intervals), 32 for one of H16 — behind the kernel's test for a plain read: any interval shorter than W, an
    end beyond the read or the key range: deferred whatever the rest says."""
    c = min(c, 0x3FFFFFFF)
    n = len(iv)
    irregular = n < 2 or any(not (0 <= s < e <= min(L, K_MAX_KEY_POS)) or e - s < W for s, e in iv)
    if irregular:
        return True
    if n <= c:
        return False  # (never more than c intervals open: the screen's own closed form, the whole read)
    return formulation.slid_window_screen_regions(list(iv), L, c, 16 if n <= 128 else NB, W, 0) is None


def _spread(lo, hi, k):
    """k positions lo <= p < hi, evenly spread, the first at lo and the last at hi - 1 (k >= 2)"""
    if k <= 0:
        return []
    if k == 1:
        return [lo]
    return [lo + (i * (hi - 1 - lo)) // (k - 1) for i in range(k)]


def chimera(n, x, y, c=0, L=L20, lo=0, hi=None, J=None, n_left=None, f_in=None, g_in=None, near=14, far_l=(40000, 240000),
            far_r=300000, spanners=0):
    """A chimera: a left pile that starts within W positions of `lo` and a right pile that ends within W positions of `hi`,
    nothing across the junction J (default L/2 + 7) but `spanners` intervals from lo to hi.
      * x of the left pile's intervals end within `near` positions in FRONT of J (at J - 1 - i % near), the others between
        lo + far_l[0] and lo + far_l[1];
      * y of the right pile's intervals start within `near` positions BEHIND J (at J + i % near), the others between hi - far_r
        and hi - far_r / 4;
      * f_in of the left pile (default: all) start inside the head window, the others 8 .. 2000 positions behind it; g_in of the
        right pile (default: all) end inside the tail window, the others 8 .. 2000 positions in front of it.
    With L = 2^20 (blocks of 2^16 positions) and J = L/2 + 7 the x ends lie in blocks 7 and 8 — half of them in either, so that
    block 7 stays safe up to c = 9 for x >= 20 —, the y starts in block 8: the kept events are m = x + y."""
    hi = L if hi is None else hi
    J = L // 2 + 7 if J is None else J
    n_left = (n - spanners) // 2 if n_left is None else n_left
    n_right = n - spanners - n_left
    f_in = n_left if f_in is None else f_in
    g_in = n_right if g_in is None else g_in
    assert 0 <= x <= n_left and 0 <= y <= n_right and 1 <= f_in + spanners and f_in <= n_left and g_in <= n_right
    ls = [lo + (i % W) for i in range(f_in)] + [lo + W + 8 + (i * 1990) // max(n_left - f_in, 1) for i in range(n_left - f_in)]
    le = _spread(lo + far_l[0], lo + far_l[1], n_left - x) + [J - 1 - (i % near) for i in range(x)]
    rs = [J + (i % near) for i in range(y)] + _spread(hi - far_r, hi - far_r // 4, n_right - y)
    re = [hi - W - 8 - (i * 1990) // max(n_right - g_in, 1) for i in range(n_right - g_in)] + [hi - (i % W) for i in range(g_in)]
    if spanners == 0:
        ls[0], re[-1] = lo, hi
    iv = [(lo, hi)] * spanners + list(zip(ls, sorted(le))) + list(zip(sorted(rs), re))
    assert len(iv) == n and all(0 <= s < e <= L for s, e in iv)
    return iv


def islands(c, k_front=0, a=40, b=40, L=L20):
    """Two holes that close within four consecutive sorted keys — the replay of several runs in one lane (sweep_filtered.h:
    cnt > 1; a lane sorts 128 / 32 = 4 keys).  c intervals span the read; pile A (a + k_front intervals) ends around position
    200 000, two islands of 40 positions follow 50 positions apart, pile B (b intervals) begins around 400 000: in key order
    ... A's last end | island 1's start, its end, island 2's start, its end | B's first start ...: both islands' starts are low
    (c intervals open), both of their ends flagged (c + 1 open).  Three holes; k_front = 0 .. 3 moves the four keys across the
    lanes' borders."""
    a += k_front
    A = [(i % W, 200000 - 7 * i) for i in range(a)]
    isl = [(300000, 300040), (300090, 300130)]
    B = [(400000 + 3 * i, L - (i % W)) for i in range(b)]
    return [(0, L)] * c + A + isl + B


def holes(c, k, n=200, L=L20):
    """k + 1 piles of n // (k + 1) intervals side by side, nothing across their borders but c spanning intervals: k holes.  Every
    pile but the first starts within 60 positions, every pile but the last ends within 60: their blocks are all kept."""
    per = (n - c) // (k + 1)
    iv = [(0, L)] * c
    for p in range(k + 1):
        cnt = per if p < k else n - c - per * k
        b0, b1 = (p * L) // (k + 1), ((p + 1) * L) // (k + 1)
        for i in range(cnt):
            s = (i % W) if p == 0 else b0 + 1000 + (i % 60)
            e = L - (i % W) if p == k else b1 - 1000 - (i % 60)
            iv.append((s, e))
    return iv


@functools.lru_cache(maxsize=None)
def cases(c):
    """the set at threshold c (one of COVS): Case(name, intervals, length, claim, guard, defer, m) — m: the kept events where
    the case states them, else None"""
    out = []

    def add(name, iv, L, claim, guard=None, defer=True, m=None):
        out.append(Case(name, tuple(iv), L, claim, guard, defer, m))

    # ---- kept events on the cap: m = 127, 128 (decided), 129, 130 (left)
    for n, x, y in ((200, 64, 63), (200, 64, 64), (256, 100, 28), (129, 64, 64)):
        add("cap n%d m%d" % (n, x + y), chimera(n, x, y, c), L20, "decided", "cap", m=x + y)
    for n, x, y in ((200, 64, 65), (256, 100, 29), (130, 65, 65)):
        add("cap n%d m%d" % (n, x + y), chimera(n, x, y, c), L20, "left", "cap", m=x + y)
    # ---- interval counts: odd n leaves the last pair half real
    for n in SIZES:
        add("size n%d" % n, chimera(n, 30, 30, c), L20, "decided", m=60)
    # n <= c (the screen's own closed form answers: never deferred), c = n - 1 (F <= c: left), c = 0xFFFFFFFF: under their own
    # thresholds, see special_cases()
    # ---- window counts, with pmin > 0 and pmax < len
    lo, hi = 70001, L20 - 50003
    win = dict(lo=lo, hi=hi, J=lo + 8 * 65536 + 7, far_l=(70000, 240000))  # (no end in block 0, where the F cases' other starts lie)
    add("window pmin>0 pmax<len", chimera(200, 40, 40, c, **win), L20, "decided", m=80)
    add("F = c + 1", chimera(200, 40, 40, c, f_in=c + 1, **win), L20, "decided", "F")
    add("G = c + 1", chimera(200, 40, 40, c, g_in=c + 1, **win), L20, "decided", "G")
    if c >= 1:  # (the smallest start is a start within W positions of itself: F = 0 does not exist)
        add("F = c", chimera(200, 40, 40, c, f_in=c, **win), L20, "left", "F")
        add("G = c", chimera(200, 40, 40, c, g_in=c, **win), L20, "left", "G")
    # ---- interval length: the shortest interval 31 (irregular: left) and 32 (taken) positions long, inside the hole
    base = chimera(199, 40, 40, c)
    add("shortest 32", base + [(L20 // 2 + 2000, L20 // 2 + 2032)], L20, "decided", "length")
    add("shortest 31", base + [(L20 // 2 + 2000, L20 // 2 + 2031)], L20, "left", "length")
    # ---- blocks
    # every near end in block 7 (unsafe: nothing is left open), every near start in block 8, one of them ON the border; block 7's
    # nearest end-holding block in front is kept too
    add("junction on a block border", chimera(200, 40, 40, c, J=L20 // 2), L20, "decided")
    # L <= 1023: a block is as wide as a window (sh = 5).  The piles' inner ends (484 .. 497) and starts (498 .. 511) share block
    # 15: every event but the windows' is kept, m = n
    for n in (65, 128):
        add("short read n%d" % n, chimera(n, n // 2, n - n // 2, c, L=1000, J=498), 1000, "decided", m=n)
    add("short read n129: the cap", chimera(129, 64, 65, c, L=1000, J=498), 1000, "left", "cap", m=129)
    # an unsafe block (8) whose nearest end-holding block (2) lies several safe blocks in front: 40 of the left pile end in block 2,
    # 20 stay open; 5 intervals start in each of blocks 4, 5, 6 (safe: 20 and more open, starts only) and end, with the 20, in
    # block 8, in front of the right pile's starts there
    J = 8 * 65536 + 1000
    left = [(i % W, 2 * 65536 + 100 + 50 * i) for i in range(40)] + [(i % W, J - 1 - i) for i in range(20)]
    mid = [(b * 65536 + 500 + 40 * i, J - 25 - 5 * (b - 4) - i) for b in (4, 5, 6) for i in range(5)]
    right = [(J + i, L20 - (i % W)) for i in range(30)] + [(L20 - 200000 + 100 * i, L20 - (i % W)) for i in range(65)]
    add("end-holding block far in front", left + mid + right, L20, "decided", m=40 + 20 + 15 + 30)
    # an unsafe block with no end in front of it: the whole left pile ends in block 8, where the right pile begins
    add("unsafe block, no end in front", chimera(160, 60, 40, c, J=J, n_left=60), L20, "decided", m=100)
    # events in the blocks behind T = span - W: a span of 12 blocks + 10 positions puts the tail window across a block border, and
    # the right pile's other ends 8 .. 2000 positions in front of it
    add("events behind T", chimera(200, 40, 40, c, lo=5, hi=5 + 12 * 65536 + 10, J=6 * 65536, g_in=c + 20), L20, "decided")
    # ---- runs
    add("two holes", holes(c, 2, 90 + c), L20, "decided", m=4 * 30)
    add("three holes", holes(c, 3, 80 + c), L20, "decided", m=6 * 20)
    for k in range(4):
        add("two runs in one lane, %d in front" % k, islands(c, k), L20, "decided", m=40 + k + 4 + 40)
    add("the tail closes the run", chimera(100, 30, 30, c, spanners=c), L20, "decided", m=60)
    half = 50
    add("abutting halves", [(i % W, L20 // 2) for i in range(half)] + [(L20 // 2, L20 - (i % W)) for i in range(half)], L20, "decided", m=100)
    add("a gap of one position", [(i % W, L20 // 2) for i in range(half)] + [(L20 // 2 + 1, L20 - (i % W)) for i in range(half)], L20,
        "decided", m=100)
    return tuple(out)


def special_cases():
    """the interval-count cases that bring their own threshold: (c, Case).  n <= c: the screen's closed form answers (the whole
    read) — never deferred, and the filter would leave it; c = n - 1: n > c, but F <= c; c = 0xFFFFFFFF (the kernels clamp it)."""
    out = []
    for n in (65, 200):
        iv = tuple(chimera(n, 20, 20, 0))
        out.append((n, Case("n = c, n%d" % n, iv, L20, "left", "n", False, None)))
        out.append((n + 5, Case("n < c, n%d" % n, iv, L20, "left", "n", False, None)))
        out.append((n - 1, Case("c = n - 1, n%d" % n, iv, L20, "left", "F", True, None)))
        out.append((0xFFFFFFFF, Case("c = u32 max, n%d" % n, iv, L20, "left", "n", False, None)))
    return out


def csr_of(reads):
    """[(intervals, length)] -> offsets u64, intervals u32[I, 2], lengths u32"""
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(iv) for iv, _ in reads])
    ivs = np.array([p for iv, _ in reads for p in iv], dtype=np.uint32).reshape(-1, 2)
    return off, ivs, np.array([L for _, L in reads], dtype=np.uint32)


def orderings(c):
    """the deferred cases at c as three batches: decided reads only, left reads only, and alternating — there a wavefront's two
    halves disagree (the shorter kind cycled to the longer one's length).  [(name, [Case])]"""
    dec = [k for k in cases(c) if k.defer and k.claim == "decided"]
    left = [k for k in cases(c) if k.defer and k.claim == "left"]
    alt = []
    for i in range(max(len(dec), len(left))):
        alt += [dec[i % len(dec)], left[i % len(left)]]
    return [("decided", dec), ("left", left), ("alternating", alt)]


def with_filler(marked, at, n_reads, filler_L=1000):
    """A batch of n_reads reads: marked[i] = (intervals u32[k, 2], length) stands at read at[i] (ascending), every other read is
    filler of 1 .. 3 intervals (0, filler_L), by read index.  Vectorised: the one-million-read batch is built in a second."""
    at = np.asarray(at, dtype=np.int64)
    assert len(at) == len(marked) and (len(at) == 0 or (at.max() < n_reads and (np.diff(at) > 0).all()))
    sizes = (np.arange(n_reads, dtype=np.int64) % 3) + 1
    for i, (iv, _) in zip(at.tolist(), marked):
        sizes[i] = len(iv)
    off = np.zeros(n_reads + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    ivs = np.empty((int(off[-1]), 2), np.uint32)
    ivs[:, 0], ivs[:, 1] = 0, filler_L
    lens = np.full(n_reads, filler_L, np.uint32)
    for i, (iv, L) in zip(at.tolist(), marked):
        ivs[int(off[i]):int(off[i + 1])] = np.asarray(iv, dtype=np.uint32).reshape(-1, 2)
        lens[i] = L
    return off, ivs, lens
