"""What tests/test_coordinates.py (CPU) and tests/test_gpu_coordinates.py (GPU) share: batches over the whole u32
coordinate range and on the edge of the event keys' range (csrc/device_common.h: key = pos << 2 | class holds positions up
to K = kMaxKeyPos = 0x3FFFFFFE; a read with a larger end goes to the exact path).  Generators only: nothing here runs the oracle or
the engine.  Every batch is seeded and made once per process."""
import functools
import itertools

import numpy as np

from cases import make_csr, make_read

K = 0x3FFFFFFE  # kMaxKeyPos
U32 = 2**32 - 1
ALL_MODES = ("regular", "abutting", "dups", "beyond", "sparse", "zero_len", "degenerate")  # make_read's, all but huge_pos


def csr_of(reads):
    """[(list of (start, end), length)] -> offsets u64, intervals u32[I, 2], lengths u32"""
    offsets = np.zeros(len(reads) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(iv) for iv, _ in reads])
    flat = itertools.chain.from_iterable(itertools.chain.from_iterable(iv for iv, _ in reads))
    intervals = np.fromiter(flat, dtype=np.uint64, count=2 * int(offsets[-1]))
    lengths = np.array([L for _, L in reads], dtype=np.uint64)
    assert (intervals.max() if intervals.size else 0) <= U32 and (lengths.max() if lengths.size else 0) <= U32
    return offsets, intervals.astype(np.uint32).reshape(-1, 2), lengths.astype(np.uint32)


def sub_batch(csr, keep):
    """the reads of `csr` where `keep` (bool per read) holds, in order"""
    offsets, intervals, lengths = csr
    n = np.diff(offsets.astype(np.int64))
    out = np.zeros(int(keep.sum()) + 1, np.uint64)
    out[1:] = np.cumsum(n[keep])
    return out, intervals[np.repeat(keep, n)], lengths[keep]


def scaled(csr, k):
    """every start, end and length times k (which must keep them within u32)"""
    offsets, intervals, lengths = csr
    iv, ln = intervals.astype(np.uint64) * np.uint64(k), lengths.astype(np.uint64) * np.uint64(k)
    assert (int(iv.max()) if iv.size else 0) <= U32 and int(ln.max()) <= U32
    return offsets, iv.astype(np.uint32), ln.astype(np.uint32)


def max_value(csr):
    return max(int(csr[1].max()) if csr[1].size else 0, int(csr[2].max()) if csr[2].size else 0)


# ---- part 2: the screens' crafted edges at 41 lengths ---------------------------------------------------------------------
SWEEP_LENGTHS = tuple(sorted(v for v in {2**k + d for k in range(20, 33) for d in (-1, 0, 1)} |
                             {K - 33, K - 1, K, K + 1, K + 2, K + 33} if v <= U32))
assert len(SWEEP_LENGTHS) == 41
WORKGROUP_LENGTHS = SWEEP_LENGTHS[SWEEP_LENGTHS.index(K) % 3::3]  # every third, K among them
BIG_LENGTHS = (2**22 + 1, K, K + 1, 2**31, U32)
SCREEN_BATCHES = ("register", "workgroup", "device_wide")


@functools.lru_cache(maxsize=None)
def screen_batch(which):
    """test_gpu_parity's crafted reads on the edges of the three screens, over SWEEP_LENGTHS / BIG_LENGTHS"""
    from test_gpu_parity import _crafted_screen_reads, _device_wide_screen_reads
    if which == "register":   # 65 .. 256 intervals: screen_reg.h, finish_compact.h, one_batch.h
        reads = _crafted_screen_reads(Ls=SWEEP_LENGTHS)
    elif which == "workgroup":  # 513 .. 16 384 intervals: screen_wg.h, screen_stream.h, sweep_filtered.h, sweep_lds.h
        reads = _crafted_screen_reads(ns=(513, 4097, 16384), Ls=WORKGROUP_LENGTHS, steps=(1, 127, 128, 129))
    else:  # more than 16 384 intervals: screen_big.h, sweep_big_trim.h, sweep_big.h
        rng = np.random.default_rng(99)
        reads = [r for L in BIG_LENGTHS for r in _device_wide_screen_reads(rng, (16385,), L)]
    return csr_of(reads)


# ---- part 3: random batches of one size class each, scaled ----------------------------------------------------------------
REGISTER_SIZES = (16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512)
WORKGROUP_SIZES = (513, 4096, 4097, 16384)
DEVICE_WIDE_SIZES = (16385,)
CLASS_SIZES = REGISTER_SIZES + WORKGROUP_SIZES + DEVICE_WIDE_SIZES
# An integer k puts the largest length on a goal only if that length divides the goal, and K, K + 1 and 2^31 share no divisor:
# each goal gets a batch of its own (same seed, lengths 500 .. top, the first read's exactly `top`).  K = 2 * 233 * 1103 * 2089,
# K + 1 = 3^2 * 7 * 11 * 31 * 151 * 331.  "u32": the largest k that keeps every value, ends beyond the read included, in u32.
GOALS = {"K": (2206, K), "K+1": (3641, K + 1), "2^31": (2048, 2**31), "u32": (4000, None)}


@functools.lru_cache(maxsize=None)
def class_batch(size, goal):
    """-> (csr at k = 1, k): reads of `size` intervals each, make_read's seven modes in turn"""
    top, target = GOALS[goal]
    R = 140 if size <= 512 else 7
    rng = np.random.default_rng(size)
    lengths = rng.integers(500, min(top, 3000) + 1, size=R)  # (3000: an abutting read's ends reach a quarter beyond its length)
    lengths[0] = top  # the first read is a regular one: it stays within its length
    csr = make_csr(31000 + size, [size] * R, ALL_MODES, lengths=lengths)
    k = U32 // max_value(csr) if target is None else target // top
    assert k * top == (target if target is not None else k * top) and int(csr[2].max()) == top
    return csr, k


# ---- part 4: one interval on the edge, the neighbours plain ---------------------------------------------------------------
EDGE_SIZES = (8, 100, 200, 400, 2000, 9000, 16385)
EDGE_LENGTHS = (K, K + 1, 2**31 + 7, U32)
EDGE_ENDS = (K - 1, K, K + 1, 2**31 - 1, 2**31, U32)
EDGE_SHAPES = (lambda E: (E - 5, E), lambda E: (E, E), lambda E: (E, E - 5), lambda E: (0, E))
NEIGHBOUR_LENGTHS = (10**6 + 3, 2**31 + 1, K - 1, K + 2)  # below and above K, alternating


def group_size(n):
    """reads per wavefront in the register classes (plan_compact.h): four up to 128 intervals, two up to 256, else one"""
    return 4 if n <= 128 else 2 if n <= 256 else 1


@functools.lru_cache(maxsize=None)
def edge_batch(n):
    """Reads of n plain intervals (start < end <= len).  One interval of one read is replaced by each of EDGE_SHAPES at each
    of EDGE_ENDS; the edited read takes every slot of its wavefront in turn, the other slots hold untouched plain reads.  All
    reads have n intervals, so the plan lists them in batch order and consecutive reads share a wavefront.  Then the two
    shapes whose length and intervals lie on different sides of K."""
    rng = np.random.default_rng(4000 + n)
    G = group_size(n)
    plain = [(make_read(rng, n, L, "regular"), L) for L in NEIGHBOUR_LENGTHS]
    reads = []
    for L in EDGE_LENGTHS:
        base = make_read(rng, n, L, "regular")
        for i, (E, shape) in enumerate(itertools.product(EDGE_ENDS, EDGE_SHAPES)):
            edited = base.copy()
            edited[(i * 37 + 1) % n] = shape(E)
            for slot in range(G):
                group = [plain[(j + slot + i) % 4] for j in range(G)]
                group[slot] = (edited, L)
                reads += group
    low = make_read(rng, n, 10**6, "regular")           # every interval inside [0, 10^6], the read far longer
    high = low.astype(np.uint64) + np.uint64(K - 10**6)  # every interval inside [K - 10^6, K], the read K long
    for slot in range(G):
        for L in (K + 1, 2**31, U32):
            group = [plain[(j + slot) % 4] for j in range(G)]
            group[slot] = (low, L)
            reads += group
        group = [plain[(j + slot + 1) % 4] for j in range(G)]
        group[slot] = (high.astype(np.uint32), K)
        reads += group
    offsets = np.arange(len(reads) + 1, dtype=np.uint64) * np.uint64(n)
    intervals = np.concatenate([iv for iv, _ in reads]).astype(np.uint32)
    return offsets, intervals, np.array([L for _, L in reads], dtype=np.uint32)


# ---- part 5: the same edge as overlap text --------------------------------------------------------------------------------
TEXT_LENGTHS = {"top": U32, "edge": K, "over": K + 1}


def edge_text(m4):
    """A few dozen overlap lines (PAF, or M4 when m4) between three reads of lengths 2^32 - 1, K and K + 1; the coordinates
    are part 4's: each of EDGE_SHAPES at each of EDGE_ENDS, on either side of a line."""
    ids = list(TEXT_LENGTHS)
    pairs = [shape(E) for E in EDGE_ENDS for shape in EDGE_SHAPES]
    lines = []
    for i, (s, e) in enumerate(pairs):
        a, b = ids[i % 3], ids[(i + 1 + i // 3) % 3]
        s2, e2 = pairs[(i * 7 + 3) % len(pairs)]
        la, lb = TEXT_LENGTHS[a], TEXT_LENGTHS[b]
        if m4:
            lines.append("%s %s 0.1 2 0 %d %d %d 1 %d %d %d\n" % (a, b, s, e, la, s2, e2, lb))
        else:
            lines.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\n" % (a, la, s, e, "+-"[i & 1], b, lb, s2, e2))
    return "".join(lines)
