"""The follow-on step's LONG-BATCH form on crafted edges, tier by tier: plan_kernel<4>, then mark_list_kernel ->
deferred_list_kernel (the deferred reads two per wavefront through the filtered exact sweep, csrc/sweep_filtered.h; what it leaves
sorted whole) -> scan_compact_kernel<4>.  By default only batches of 400 000 reads and more take it; Engine.debug_long_min_reads(0)
gives it every batch.  Every case is the oracle's bytes AND who decided the deferred reads: timing()["deferred_reads"] against the
screen's emulation, debug_counters()["deferred_sorted"] against the filtered sweep's.  The reads and their claims are
tests/follow_on_cases.py's; tests/test_follow_on_cases.py holds the claims against the CPU emulations."""
import functools

import numpy as np
import pytest

import follow_on_cases as fc
import oracle
import yacrd_amd
from cases import assert_same
from test_gpu_parity import _crafted_screen_reads, _prediction_batches, _region_outgrowing_inputs

pytestmark = pytest.mark.gpu

# the long launch's screen (two items per wavefront: no second looks), every verdict counted
FLAGS = yacrd_amd.F_ALWAYS_DEFER | yacrd_amd.F_SCREEN_ITEMS_2 | yacrd_amd.F_COUNT_PREFILTERED
assert FLAGS == fc.F_ALWAYS_DEFER | fc.F_SCREEN_ITEMS_2 | fc.F_COUNT_PREFILTERED and yacrd_amd.F_SCREEN_DIRECT == fc.F_SCREEN_DIRECT
K_LIST_THREADS, K_LIST_OCC = 512, 6  # kListThreads, YK_LIST_OCC (csrc/finish_compact.h): deferred_list_kernel's grid is
#                                      CUs * (K_LIST_OCC * 256 / K_LIST_THREADS) workgroups, which take 512 list entries per turn
K_MARK_READS, K_DEFER_SHARDS = 4096, 256  # kMarkReads, kDeferShards


def long_engine(flags=FLAGS):
    e = yacrd_amd.Engine(device_id=0, flags=flags)
    e.debug_long_min_reads(0)
    return e


def want_of(csr, c, threads=8):
    return oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), c, 0.4, n_threads=threads)


def tiers(e):
    """(reads the screen deferred, of those: sorted whole, decided by the filtered sweep)"""
    d, s = e.timing()["deferred_reads"], e.debug_counters()["deferred_sorted"]
    return d, s, d - s


def check_tiers(e, csr, c, want, deferred, left, ctx):
    assert_same(e.run(*csr, c, 0.4), want, ctx)
    d, s, f = tiers(e)
    print("%s: deferred %d (emulation %d), sorted whole %d (emulation %d), filtered %d" % (ctx, d, deferred, s, left, f))
    assert d == deferred, (ctx, "deferred_reads", d, deferred)
    assert s == left, (ctx, "deferred_sorted", s, left)
    assert f == deferred - left, ctx


def emulated(reads, c):
    """(reads the screen's emulation defers, of those: reads the filtered sweep's emulation leaves)"""
    deferred = [iv_L for iv_L in reads if fc.screen_defers(iv_L[0], iv_L[1], c)]
    return len(deferred), sum(1 for iv, L in deferred if fc.filtered(iv, L, c)[0] is None)


# ---- (a) the guards, tier by tier
@functools.lru_cache(maxsize=None)
def ordered_batch(c, which):
    ks = dict(fc.orderings(c))[which]
    reads = [(k.iv, k.L) for k in ks]
    csr = fc.csr_of(reads)
    return csr, want_of(csr, c), emulated(reads, c), sum(1 for k in ks if k.claim == "left")


@pytest.mark.parametrize("c", fc.COVS)
def test_guards_tier_by_tier(c):
    """the cases in three orders of the list — decided reads only, left reads only, alternating (a wavefront's two halves
    disagree) —: the screen's emulation says how many are deferred, the filtered sweep's how many of those are sorted whole"""
    with long_engine() as e:
        for which in ("decided", "left", "alternating"):
            csr, want, (deferred, left), claimed_left = ordered_batch(c, which)
            assert deferred == len(csr[2]) and left == claimed_left  # (what tests/test_follow_on_cases.py holds case by case)
            for run in range(2):
                check_tiers(e, csr, c, want, deferred, left, "c %d %s run %d" % (c, which, run))


def test_interval_counts_against_the_threshold():
    """n <= c: the screen's own closed form (not deferred); c = n - 1: deferred and left; c = 0xFFFFFFFF"""
    reads = sorted({(k.iv, k.L) for _, k in fc.special_cases()})
    csr = fc.csr_of(reads)
    with long_engine() as e:
        for c in sorted({c for c, _ in fc.special_cases()}):
            deferred, left = emulated(reads, c)
            check_tiers(e, csr, c, want_of(csr, c), deferred, left, "c %d" % c)


@pytest.mark.parametrize("flags", [yacrd_amd.F_SCREEN_DIRECT, 0], ids=["direct", "default"])
@pytest.mark.parametrize("c", fc.COVS)
def test_guard_batches_parity_on_other_builds(c, flags):
    with long_engine(flags) as e:
        for which in ("decided", "left", "alternating"):
            csr, want, _, _ = ordered_batch(c, which)
            assert_same(e.run(*csr, c, 0.4), want, "c %d %s flags %d" % (c, which, flags))
        if flags == yacrd_amd.F_SCREEN_DIRECT:
            assert e.direct_runs() >= 3  # (F_SCREEN_DIRECT: at any batch size; a batch run again after a missed prediction counts twice)


# ---- (b) the list's shape: chimeras are the marked reads, reads of 1 to 3 intervals the filler
@functools.lru_cache(maxsize=None)
def pool(c):
    return [((np.array(k.iv, np.uint32), k.L), k.claim == "left") for k in dict(fc.orderings(c))["alternating"]]


def marked_batch(c, at, n_reads):
    p = pool(c)
    picked = [p[i % len(p)] for i in range(len(at))]
    return fc.with_filler([m for m, _ in picked], at, n_reads), len(at), sum(1 for _, left in picked if left)


def run_marked(e, c, at, n_reads, ctx, threads=8):
    csr, deferred, left = marked_batch(c, at, n_reads)
    check_tiers(e, csr, c, want_of(csr, c, threads), deferred, left, ctx)


@pytest.mark.parametrize("marked", [0, 1, 2, 3, 511, 512, 513, 1025])
def test_list_lengths(marked):
    """an odd total leaves a lone read in the last pair; 513 and 1025 are more than a 512-entry turn holds, dealt out over the grid"""
    n_reads = 4099  # (n_reads % 4 == 3: the last thread of scan_compact_kernel<4> and mark_list_kernel takes the scalar path)
    at = np.unique(np.linspace(0, n_reads - 1, marked).astype(np.int64)) if marked else np.zeros(0, np.int64)
    assert len(at) == marked
    with long_engine() as e:
        run_marked(e, 3, at, n_reads, "marked %d" % marked)


@pytest.mark.parametrize("n_reads", [1, 3, 4095, 4096, 4097, 8190])
def test_batch_sizes(n_reads):
    at = np.unique(np.concatenate([np.arange(0, n_reads, 97), [n_reads - 1]]).astype(np.int64))
    with long_engine() as e:
        run_marked(e, 3, at, n_reads, "n_reads %d" % n_reads)
        run_marked(e, 0, at[::2], n_reads, "n_reads %d again" % n_reads)


@pytest.mark.parametrize("first", [True, False])
def test_a_slab_all_marked_beside_a_slab_with_none(first):
    at = np.arange(K_MARK_READS, dtype=np.int64) + (0 if first else K_MARK_READS)
    with long_engine() as e:
        run_marked(e, 3, at, 2 * K_MARK_READS, "first slab marked" if first else "second slab marked")


def test_more_slabs_than_shards():
    """1 048 577 + 4096 reads: 258 slabs of 4096 on 256 shards, so slabs 256 and 257 add to shards 0 and 1; a few hundred marked
    reads in the first, the middle and the last slabs"""
    n_reads = 1048577 + 4096
    slabs = -(-n_reads // K_MARK_READS)
    assert slabs > K_DEFER_SHARDS + 1
    at = []
    for slab in (0, 1, slabs // 2, K_DEFER_SHARDS - 1, K_DEFER_SHARDS, slabs - 1):
        lo, hi = slab * K_MARK_READS, min((slab + 1) * K_MARK_READS, n_reads)
        at += list(range(lo, hi, max((hi - lo) // 60, 1)))[:60] + [hi - 1]
    at = np.unique(np.array(at, dtype=np.int64))
    assert 200 < len(at) < 500 and at[-1] == n_reads - 1
    with long_engine() as e:
        run_marked(e, 0, at, n_reads, "1 M reads", threads=16)


# ---- (c) the second turn of a workgroup's list
def test_second_turn_of_a_workgroups_list():
    """400 000 chimeras of 65 intervals, no debug_long_min_reads: long by the DEFAULT threshold.  Half of them built to be decided
    by the filtered sweep, half to be left (F = c, G = c, an interval of 31 positions), interleaved.  Every read is marked, so a
    workgroup of deferred_list_kernel's grid takes ceil(400 000 / grid) > 512 entries: its c0 loop comes round a second time."""
    n_reads, n, c = 400000, 65, 3
    win = dict(far_l=(70000, 240000))
    # (with c intervals across the junction its block is entered at D - E = c exactly: ON the unsafe-block rule, not beyond it)
    dec = [fc.chimera(n, x, y, c, spanners=sp) for x, y, sp in ((20, 20, 0), (25, 30, c), (30, 25, 0), (31, 31, c))]
    left = [fc.chimera(n, 20, 20, c, f_in=c, **win), fc.chimera(n, 20, 20, c, g_in=c, **win),
            fc.chimera(n - 1, 20, 20, c) + [(fc.L20 // 2 + 2000, fc.L20 // 2 + 2031)]]
    for iv in dec + left:
        assert len(iv) == n and fc.screen_defers(iv, fc.L20, c) and (fc.filtered(iv, fc.L20, c)[0] is None) == (iv in left)
    T = np.array(dec + left, dtype=np.uint32)  # [7, 65, 2]
    r = np.arange(n_reads)
    which = np.where(r % 2 == 0, (r // 2) % len(dec), len(dec) + (r // 2) % len(left))
    csr = (np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(n), T[which].reshape(-1, 2), np.full(n_reads, fc.L20, np.uint32))
    want = want_of(csr, c, threads=16)
    with yacrd_amd.Engine(device_id=0, flags=FLAGS) as e:
        grid = e.compute_units() * (K_LIST_OCC * 256 // K_LIST_THREADS)
        assert grid > 0 and -(-n_reads // grid) > K_LIST_THREADS, (grid, "the batch no longer reaches the second turn")
        check_tiers(e, csr, c, want, n_reads, n_reads // 2, "400 000 chimeras")


# ---- (d) the redo of the follow-on step after a region-buffer overflow
def concat_csr(parts):
    off = [np.zeros(1, np.uint64)]
    for o, _, _ in parts:
        off.append(o[1:] + off[-1][-1])
    return np.concatenate(off), np.concatenate([iv for _, iv, _ in parts]), np.concatenate([ln for _, _, ln in parts])


@functools.lru_cache(maxsize=None)
def outgrowing_inputs():
    return tuple(_region_outgrowing_inputs())


@pytest.mark.parametrize("flags", [0, FLAGS], ids=["default", "screened"])
def test_region_buffer_outgrown_on_the_long_form(flags):
    """tests/test_gpu_parity.py's four inputs: the first run of a fresh engine outgrows bad_regions and redoes the follow-on step;
    the redo lists what is still marked — nothing: the count of deferred reads does not double"""
    for n_reads, per_read, cov, csr, want in outgrowing_inputs():
        n = per_read * (2 if cov else 1)
        deferred = n_reads if (flags and 65 <= n <= 256) else 0  # (disjoint intervals of 1 .. 9 positions: irregular, every one sorted whole)
        with long_engine(flags) as e:
            for run in range(2):
                ctx = "%d x %d run %d" % (n_reads, per_read, run)
                if flags:
                    check_tiers(e, csr, cov, want, deferred, deferred, ctx)
                else:
                    assert_same(e.run(*csr, cov, 0.4), want, ctx)
                    assert e.timing()["deferred_reads"] == 0


def test_redo_with_marked_reads():
    """the four inputs and marked chimeras in one batch, twice on a fresh engine: the first run redoes the follow-on step"""
    c = 0
    p = pool(c)
    chim, n_left = [], 0
    for g in range(3):
        picked = [p[(200 * g + i) % len(p)] for i in range(200)]
        n_left += sum(1 for _, left in picked if left)
        chim.append(fc.csr_of([(m[0].tolist(), m[1]) for m, _ in picked]))
    ins = [csr for _, _, _, csr, _ in outgrowing_inputs()]
    csr = concat_csr([chim[0], ins[0], chim[1], ins[1], ins[2], chim[2], ins[3]])
    want = want_of(csr, c)
    assert int(want[0][-1]) > 4 * len(csr[2]) + 1024
    with long_engine() as e:
        for run in range(2):
            check_tiers(e, csr, c, want, 600 + 1500, n_left + 1500, "mixed run %d" % run)


# ---- (e) the existing crafted sets on the long form
@pytest.mark.parametrize("cov", [0, 3, 4, 0xFFFFFFFF])
def test_healthy_screen_edges_on_the_long_form(cov):
    reads = _crafted_screen_reads()
    csr = fc.csr_of(reads)
    want = want_of(csr, cov)
    with long_engine() as e:
        assert_same(e.run(*csr, cov, 0.4), want, "cov %d" % cov)
        d, s, f = tiers(e)
        assert 0 < s <= d and e.timing()["prefiltered_reads"] > 0


@pytest.mark.parametrize("flags", [0, yacrd_amd.F_ALWAYS_DEFER, yacrd_amd.F_ALWAYS_DEFER | yacrd_amd.F_SCREEN_ITEMS_2])
def test_class_prediction_on_the_long_form(flags):
    """the same predicted / prediction_misses sequence as on the short form"""
    seen = {True: [], False: []}
    with long_engine(flags) as e, yacrd_amd.Engine(device_id=0, flags=flags) as short:
        for rep, csr, want in _prediction_batches():
            for eng, is_long in ((e, True), (short, False)):
                assert_same(eng.run(*csr, 3, 0.4), want, "run %d long %d" % (rep, is_long))
                t = eng.timing()
                seen[is_long].append((t["predicted"], t["prediction_misses"]))
    assert seen[True] == seen[False] and any(p for p, _ in seen[True]) and any(m for _, m in seen[True]), seen
