"""The long launch taking its H16 reads BY INDEX (screen_reg.h: screen_block_rows, DIRECT): rows = reads 4 b .. 4 b + 3, a row
whose read is not H16 idle, the plan and every other class beside the launch on the engine's side stream, the read's count
word written by the screen.  Through the C ABI with F_SCREEN_DIRECT (direct wherever it is legal, at any batch size), bit-exact
against the CPU oracle; and the same reads deferred as by the list form (F_ALWAYS_DEFER | F_SCREEN_ITEMS_2 |
F_NO_SCREEN_DIRECT): one form of the screen, the same verdicts.  The GPU tests need an MI355X."""
import os
import re

import numpy as np
import pytest

import oracle
import yacrd_amd
from cases import assert_same

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = yacrd_amd.F_SCREEN_DIRECT
LISTED = yacrd_amd.F_ALWAYS_DEFER | yacrd_amd.F_SCREEN_ITEMS_2 | yacrd_amd.F_NO_SCREEN_DIRECT
COVS = [0, 1, 3, 4, 9]


# ---- the H16 rule, restated once ---------------------------------------------------------------------------------------
def is_h16(n, lo=129, hi=256):
    """a read of n intervals is of class H16: 128 < n <= 256"""
    return lo <= n <= hi


# ---- reads --------------------------------------------------------------------------------------------------------------
def pile(rng, n, L, lo=None, gap=None, exact=False):
    """A healthy pile-up of n >= 3 intervals on a read of length L >= 5000 (test_gpu_screen_h16_rows.py: pile): a third
    dovetails from the left starting within 16 positions of lo, a third dovetails to the right ending within 16 positions of
    L - gap, the rest inside; every interval spans the middle.  exact: the dovetails start at lo / end at L - gap exactly,
    so the read's regions are (0, lo) if lo > 0 and (L - gap, L) if gap > 0 and nothing else (c < n // 3)."""
    k = n // 3
    lo = int(rng.integers(0, 300)) if lo is None else lo
    hi = L - (int(rng.integers(0, 300)) if gap is None else gap)
    j = (lambda m: np.zeros(m, np.int64)) if exact else (lambda m: rng.integers(0, 16, m))
    s = np.concatenate([lo + j(k), lo + 150 + rng.integers(0, 50, k), lo + 120 + rng.integers(0, 100, n - 2 * k)])
    e = np.concatenate([hi - 200 - rng.integers(0, 50, k), hi - j(k), hi - 120 - rng.integers(0, 100, n - 2 * k)])
    iv = np.stack([s, e], axis=1)
    return iv[rng.permutation(n)].astype(np.uint32)


def chimera(rng, n, L):
    """two abutting halves: every interval stops in front of the middle or starts behind it — the screen defers the read"""
    iv = pile(rng, n, L).astype(np.int64)
    left = np.arange(n) % 2 == 0
    iv[left, 1] = L // 2 - 10 - np.arange(n)[left] % 20
    iv[~left, 0] = L // 2 + 10 + np.arange(n)[~left] % 20
    return iv.astype(np.uint32)


def to_csr(reads):
    """reads: [(intervals u32[n, 2], length)] -> offsets u64, intervals u32[I, 2], lengths u32"""
    offsets = np.zeros(len(reads) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(iv) for iv, _ in reads])
    return offsets, np.concatenate([iv for iv, _ in reads]).astype(np.uint32), np.array([L for _, L in reads], np.uint32)


# ---- the check every case goes through -----------------------------------------------------------------------------------
class Pair:
    """one engine that goes direct and one that takes the list form, for a module's worth of cases"""

    def __init__(self):
        self.direct = yacrd_amd.Engine(flags=DIRECT)
        self.listed = yacrd_amd.Engine(flags=LISTED)
        self.shape = None  # (reads, intervals) of the direct engine's last batch: what its prediction is keyed by

    def close(self):
        self.direct.close()
        self.listed.close()

    def check(self, csr, cov, ctx):
        """Three runs on the direct engine — the first without a prediction (unless the batch before had this very shape),
        two with —, every one direct and the oracle's; then the list form: the oracle's again and the same reads deferred."""
        want = oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), cov, 0.4, n_threads=4)
        shape = (len(csr[2]), int(csr[0][-1]))
        # (a read beyond 16 384 intervals that the device-wide screen leaves to the host is never predicted: engine.hip)
        has_big = bool((np.diff(csr[0].astype(np.int64)) > 16384).any())
        deferred = []
        for k in range(3):
            before = self.direct.direct_runs()
            assert_same(self.direct.run(*csr, cov, 0.4), want, "%s, direct run %d" % (ctx, k))
            t = self.direct.timing()
            assert self.direct.direct_runs() > before, (ctx, k)
            assert has_big or t["predicted"] == (1 if k or shape == self.shape else 0), (ctx, k, t["predicted"])
            assert t["screen_items"] == 2, (ctx, k, t["screen_items"])
            deferred.append(t["deferred_reads"])
        self.shape = shape
        assert_same(self.listed.run(*csr, cov, 0.4), want, "%s, list form" % ctx)
        t = self.listed.timing()
        assert self.listed.direct_runs() == 0
        assert deferred == [t["deferred_reads"]] * 3, (ctx, deferred, t["deferred_reads"])
        return t["deferred_reads"]


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    p.close()


# ---- 1. row activity -----------------------------------------------------------------------------------------------------
# interval counts per read: batches of 1, 2, 3, 4, 5, 7 and 9 reads (partial last wavefronts); a non-H16 read in every row
# of a wavefront in turn; a batch without an H16 read (no row of the launch active); a batch of H16 reads only
ROW_BATCHES = [
    [199], [128],
    [257, 129], [130, 3],
    [255, 40, 256], [64, 65, 128],
    [129, 130, 255, 256],
    [128, 199, 255, 256], [129, 257, 199, 130], [256, 255, 600, 129], [130, 199, 129, 5000],
    [199, 20000, 256, 129, 64],
    [129, 3, 40, 255, 256, 65, 130],
    [600, 199, 256, 257, 5000, 129, 255, 128, 130],
]


def test_row_batches_cover_what_they_claim():
    used = {n for b in ROW_BATCHES for n in b}
    assert used == {3, 40, 64, 65, 128, 129, 130, 199, 255, 256, 257, 600, 5000, 20000}
    assert sorted({len(b) for b in ROW_BATCHES}) == [1, 2, 3, 4, 5, 7, 9]
    assert any(not any(is_h16(n) for n in b) for b in ROW_BATCHES) and any(all(is_h16(n) for n in b) for b in ROW_BATCHES)
    idle_rows = {i % 4 for b in ROW_BATCHES if any(is_h16(n) for n in b) for i, n in enumerate(b) if not is_h16(n)}
    assert idle_rows == {0, 1, 2, 3}


@gpu
@pytest.mark.parametrize("cov", COVS)
def test_row_activity(pair, cov):
    """Every batch three ways: healthy piles only (the closed-form sink beside idle rows), chimeras at the odd reads and at
    the even reads (the deferring sink beside them)."""
    rng = np.random.default_rng(5100 + cov)
    for b, sizes in enumerate(ROW_BATCHES):
        for variant in range(3):
            reads = []
            for i, n in enumerate(sizes):
                L = int(rng.integers(30000, 60000))
                reads.append((chimera(rng, n, L) if variant and i % 2 == variant - 1 else pile(rng, n, L), L))
            pair.check(to_csr(reads), cov, "batch %d variant %d c %d" % (b, variant, cov))


# ---- 2. the count word ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cov", COVS)
def test_count_word(pair, cov):
    """H16 reads decided with no region (the count 0 in four bytes), with one and with two (closed[r] and the kClosedForm
    word, both written by the screen while the plan writes its neighbours' words), beside deferred reads and reads of the
    other classes, whose words are the plan's."""
    rng = np.random.default_rng(5200 + cov)
    kinds = ["none", "left", "right", "two", "chimera", "r16", "w16", "m1", "r8"]
    order = [kinds[i] for i in rng.permutation(np.arange(45) % len(kinds))]
    reads, regions = [], []
    for kind in order:
        L = int(rng.integers(30000, 60000))
        n = int(rng.integers(129, 257))
        if kind == "none": reads.append((pile(rng, n, L, 0, 0, exact=True), L)), regions.append(0)
        elif kind == "left": reads.append((pile(rng, n, L, 77, 0, exact=True), L)), regions.append(1)
        elif kind == "right": reads.append((pile(rng, n, L, 0, 91, exact=True), L)), regions.append(1)
        elif kind == "two": reads.append((pile(rng, n, L, 77, 91, exact=True), L)), regions.append(2)
        elif kind == "chimera": reads.append((chimera(rng, n, L), L)), regions.append(None)
        else:
            n = {"r16": 100, "w16": 300, "m1": 600, "r8": 50}[kind]
            reads.append((pile(rng, n, L), L)), regions.append(None)
    csr = to_csr(reads)
    want = oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), cov, 0.4, n_threads=4)
    got = np.diff(want[0].astype(np.int64))
    for r, k in enumerate(regions):  # (the generator does what it says: the oracle's counts)
        assert k is None or got[r] == k, (r, order[r], int(got[r]), k)
    deferred = pair.check(csr, cov, "count word c %d" % cov)
    assert order.count("chimera") <= deferred < sum(k in ("none", "left", "right", "two", "chimera", "r16") for k in order)


# ---- 3. prediction ---------------------------------------------------------------------------------------------------------
def _uniform(rng, sizes):
    return to_csr([(pile(rng, n, 40000), 40000) for n in sizes])


@gpu
def test_prediction_miss_then_hit():
    """Two shapes of the same reads and intervals on one engine, A, B, A, A: B is predicted with A's classes (H16 only) and
    holds an M1 read and four R16 reads besides — a miss, recovered; A behind B is a hit (B's classes cover it)."""
    rng = np.random.default_rng(5300)
    a_sizes = [200] * 2000
    b_sizes = list(a_sizes)
    b_sizes[5] = 600
    b_sizes[6:10] = [100] * 4
    assert sum(a_sizes) == sum(b_sizes)
    A, B = _uniform(rng, a_sizes), _uniform(rng, b_sizes)
    wants = {id(x): oracle.run(x[0], x[1], x[2].astype(np.uint64), 3, 0.4, n_threads=4) for x in (A, B)}
    with yacrd_amd.Engine(flags=DIRECT) as e:
        seen = []
        for k, x in enumerate((A, B, A, A)):
            before = e.direct_runs()
            assert_same(e.run(*x, 3, 0.4), wants[id(x)], "A B A A, run %d" % k)
            assert e.direct_runs() > before, k
            t = e.timing()
            seen.append((t["predicted"], t["prediction_misses"]))
        assert seen == [(0, 0), (1, 1), (1, 0), (1, 0)], seen


@gpu
def test_default_rule_and_the_force_flag():
    """Without the force flag (the long-launch build pinned): a batch whose H16 share is below 7/8, and a batch of 2 000 H16
    reads with one M1 read, do not go direct.  With it the second does: H16 by index, the M1 read through its own path."""
    rng = np.random.default_rng(5400)
    mixed = _uniform(rng, [200, 100, 200, 300] * 300)  # half H16
    with_m1 = _uniform(rng, [200] * 1000 + [600] + [200] * 1000)
    pinned = yacrd_amd.F_ALWAYS_DEFER | yacrd_amd.F_SCREEN_ITEMS_2
    for name, csr in (("half H16", mixed), ("one M1 read", with_m1)):
        want = oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), 3, 0.4, n_threads=4)
        with yacrd_amd.Engine(flags=pinned) as e:
            for k in range(3):
                assert_same(e.run(*csr, 3, 0.4), want, "%s, default rule, run %d" % (name, k))
            assert e.direct_runs() == 0, name
            deferred = e.timing()["deferred_reads"]
        with yacrd_amd.Engine(flags=DIRECT) as e:
            for k in range(3):
                assert_same(e.run(*csr, 3, 0.4), want, "%s, forced, run %d" % (name, k))
                assert e.timing()["deferred_reads"] == deferred, (name, k)
            assert e.direct_runs() == 3, name
            if name == "one M1 read":
                assert e.timing()["class_reads"][9] == 1  # (CLS_MED1: the read went its own way)


# ---- 4. pipelined ------------------------------------------------------------------------------------------------------------
@gpu
def test_pipelined_over_two_engines():
    """Six batches of generated Sequel reads, a tenth of them chimeras, over two direct engines in flight; what the engines
    held is gone when they are closed."""
    import torch
    from yacrd_amd import host
    from yacrd_amd.engine import live_bytes
    live_before = live_bytes()
    batches = [host.synth_csr(host.SYNTH_SEQUEL, 2000 + 37 * i, 200000 + 3700 * i, 5500 + i, flags=host.synth_f_chimera_pct(10))
               for i in range(6)]
    wants = [oracle.run(b[0], b[1], b[2].astype(np.uint64), 3, 0.4, n_threads=4) for b in batches]
    dev = torch.device("cuda", 0)
    keep, dev_batches = [], []
    for o, iv, ln in batches:
        t = [torch.from_numpy(x).to(dev) for x in (o.view(np.int64), iv.view(np.int32).reshape(-1), ln.view(np.int32))]
        keep.append(t)
        dev_batches.append((t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(ln), int(o[-1]), 3, 0.4))
    torch.cuda.synchronize()
    engs = [yacrd_amd.Engine(flags=DIRECT) for _ in range(2)]
    try:
        yacrd_amd.run_device_batches(engs, dev_batches, lambda i, e: assert_same(e.fetch(), wants[i], "pipelined batch %d" % i))
        for e in engs:
            assert e.direct_runs() >= 3, e.direct_runs()
    finally:
        for e in engs:
            e.close()
    assert live_bytes() == live_before


# ---- 5. one predicate (no GPU) -------------------------------------------------------------------------------------------
def _header(name):
    with open(os.path.join(ROOT, "yacrd_amd", "csrc", name)) as f:
        return f.read()


def test_plan_rule_and_row_activity_are_one_predicate():
    """plan_kernel's mode-0 rule for H16 (plan_compact.h: above R16's 2 n <= 256, up to 2 n <= 512) and the direct launch's
    row activity (screen_reg.h: kH16MinIntervals <= n <= kH16MaxIntervals) say the same of every n in 0..600 — and what this
    file's restatement says."""
    plan = _header("plan_compact.h")
    r16 = re.search(r"m <= (\d+)\) c = CLS_R16;", plan)
    h16 = re.search(r"mode == 0 && m <= (\d+)\) c = CLS_H16;", plan)
    assert r16 and h16
    m_lo, m_hi = int(r16.group(1)), int(h16.group(1))
    rows = re.search(r"kH16MinIntervals = (\d+), kH16MaxIntervals = (\d+);", _header("screen_reg.h"))
    assert rows
    lo, hi = int(rows.group(1)), int(rows.group(2))
    assert re.search(r"return n >= \(u64\)kH16MinIntervals && n <= \(u64\)kH16MaxIntervals;", _header("screen_reg.h"))
    for n in range(601):
        by_plan = m_lo < 2 * n <= m_hi
        assert by_plan == is_h16(n, lo, hi) == is_h16(n) == (128 < n <= 256), n
