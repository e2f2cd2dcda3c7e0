"""The long launch's H16 form (screen_reg.h: H16 ROWS): an H16 read on one 16-lane row, sixteen intervals per lane,
32 coarse blocks two per lane, four reads per wavefront as ONE item.  Through the C ABI with F_ALWAYS_DEFER |
F_SCREEN_ITEMS_2 (the long-launch build at any batch size), bit-exact against the CPU oracle.  Needs an MI355X."""
import numpy as np
import pytest

import oracle
import yacrd_amd
from cases import assert_same, make_read

pytestmark = pytest.mark.gpu

TWO = yacrd_amd.F_ALWAYS_DEFER | yacrd_amd.F_SCREEN_ITEMS_2
ONE = yacrd_amd.F_ALWAYS_DEFER | yacrd_amd.F_SCREEN_ITEMS_1


@pytest.fixture(scope="module")
def engine2():
    with yacrd_amd.Engine(flags=TWO) as e:
        yield e


def pile(rng, n, L):
    """A healthy pile-up of n >= 33 intervals on a read of length L >= 5000: a third of them dovetails from the left whose
    starts lie within 16 positions of each other, a third dovetails to the right whose ends do, the rest inside; every
    interval spans the read's middle, so the read is bad in front of its (c+1)-th start and behind its (c+1)-th largest
    end only (c <= 9).  The piles stand a random distance inside the read: pmin > 0 and pmax < len for most reads."""
    k = n // 3
    lo, hi = int(rng.integers(0, 300)), L - int(rng.integers(0, 300))
    s = np.concatenate([lo + rng.integers(0, 16, k), lo + 150 + rng.integers(0, 50, k), lo + 120 + rng.integers(0, 100, n - 2 * k)])
    e = np.concatenate([hi - 200 - rng.integers(0, 50, k), hi - rng.integers(0, 16, k), hi - 120 - rng.integers(0, 100, n - 2 * k)])
    iv = np.stack([s, e], axis=1)
    return iv[rng.permutation(n)].astype(np.uint32)


def to_csr(reads):
    """reads: [(intervals u32[n, 2], length)] -> offsets u64, intervals u32[I, 2], lengths u32"""
    offsets = np.zeros(len(reads) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(iv) for iv, _ in reads])
    return offsets, np.concatenate([iv for iv, _ in reads]).astype(np.uint32), np.array([L for _, L in reads], np.uint32)


def check(e, csr, cov, ctx):
    want = oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), cov, 0.4, n_threads=4)
    got = e.run(*csr, cov, 0.4)
    assert_same(got, want, ctx)
    t = e.timing()
    assert t["screen_items"] == 2, t  # the long-launch build ran
    return got, t


# ---- 1. lane-layout edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cov", [0, 1, 3, 4, 9])
def test_lane_layout_edges(engine2, cov):
    """Batches of 1..7 reads (5 and 7: a partial last wavefront) of n = 129..256 intervals (odd n: the clamped last pair;
    256: every slot of the row real; 129 / 130: seven of a lane's eight pairs are copies): healthy piles, every read
    decided by the screen in closed form."""
    rng = np.random.default_rng(4100 + cov)
    for batch in (1, 2, 3, 4, 5, 7):
        for n in (129, 130, 131, 199, 200, 255, 256):
            reads = [(pile(rng, n, L), L) for L in rng.integers(5000, 60000, size=batch).tolist()]
            _, t = check(engine2, to_csr(reads), cov, "batch %d n %d c %d" % (batch, n, cov))
            assert t["deferred_reads"] == 0, (batch, n, cov, t["deferred_reads"])
    # and the sizes side by side in one batch: neighbours in a wavefront with different clamps
    sizes = [129, 256, 131, 200, 255, 130, 199, 256, 129, 255, 131]
    reads = [(pile(rng, n, 5000 + 977 * i), 5000 + 977 * i) for i, n in enumerate(sizes)]
    _, t = check(engine2, to_csr(reads), cov, "sizes side by side c %d" % cov)
    assert t["deferred_reads"] == 0, t["deferred_reads"]


# ---- 2. mixed groups in one wavefront ------------------------------------------------------------------------------
def _irregular(kind, rng, n, L):
    iv = pile(rng, n, L).astype(np.int64)
    if kind == "chimera":        # one hole: every interval stops in front of the middle or starts behind it
        left = np.arange(n) % 2 == 0
        iv[left, 1] = L // 2 - 10 - np.arange(n)[left] % 20
        iv[~left, 0] = L // 2 + 10 + np.arange(n)[~left] % 20
    elif kind == "short_window":  # three starts inside the head window (c = 3 needs four), the others spread behind it
        order = np.argsort(iv[:, 0], kind="stable")
        base = int(iv[order[0], 0])
        iv[order[:3], 0] = base + np.array([0, 5, 10])
        iv[order[3:], 0] = base + 40 + 3 * np.arange(n - 3)
    elif kind == "short_interval":
        iv[7] = (L // 3, L // 3 + 20)
    elif kind == "zero_length":
        iv[7] = (L // 3, L // 3)
    elif kind == "reversed":
        iv[7] = (L // 3 + 100, L // 3)
    elif kind == "beyond_len":
        iv[7] = (L // 3, L + 5)
    else:
        raise ValueError(kind)
    return iv.astype(np.uint32)


@pytest.mark.parametrize("kind", ["chimera", "short_window", "short_interval", "zero_length", "reversed", "beyond_len"])
def test_one_irregular_read_among_healthy_neighbours(engine2, kind):
    """Four consecutive H16 reads = one wavefront, one row each: the irregular read (in each of the four rows in turn) is
    deferred, and it alone — its neighbours' tables are their own; then two wavefronts with one such read in each."""
    rng = np.random.default_rng(4200)
    cov = 3
    for n in (200, 131, 256):
        for where in range(4):
            reads = []
            for i in range(4):
                L = int(rng.integers(8000, 60000))
                reads.append((_irregular(kind, rng, n, L) if i == where else pile(rng, n, L), L))
            _, t = check(engine2, to_csr(reads), cov, "%s in row %d n %d" % (kind, where, n))
            assert t["deferred_reads"] == 1, (kind, where, n, t["deferred_reads"])
    reads = []
    for i in range(8):
        L = int(rng.integers(8000, 60000))
        reads.append((_irregular(kind, rng, 180 + i, L) if i in (1, 6) else pile(rng, 180 + i, L), L))
    _, t = check(engine2, to_csr(reads), cov, "%s in two wavefronts" % kind)
    assert t["deferred_reads"] == 2, (kind, t["deferred_reads"])


# ---- 3. mixed classes ------------------------------------------------------------------------------------------------
def test_classes_interleaved(engine2):
    """R8, R16, H16 and W16 reads interleaved (the H16 list is not contiguous in read id), healthy piles next to reads
    of every regular mode: the launch holds sorting classes, R16's two items of four reads and H16's rows on one table."""
    rng = np.random.default_rng(4300)
    modes = ("regular", "abutting", "dups", "beyond", "sparse", "zero_len", "degenerate")
    bounds = ((33, 64), (65, 128), (129, 256), (257, 512))
    reads, in_screen = [], 0
    for r in range(3000):
        lo, hi = bounds[int(rng.integers(0, 4))]
        n = int(rng.integers(lo, hi + 1))
        L = int(rng.integers(5000, 60000))
        in_screen += 65 <= n <= 256
        reads.append((pile(rng, n, L) if r % 3 else make_read(rng, n, L, modes[(r // 3) % len(modes)]), L))
    for cov in (3, 0):
        _, t = check(engine2, to_csr(reads), cov, "classes interleaved c %d" % cov)
        assert 0 < t["deferred_reads"] < in_screen, (t["deferred_reads"], in_screen)  # decided and deferred reads


# ---- 4. the same decisions as the 32-lane form -------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0, 100])
def test_same_decisions_as_the_32_lane_form(sigma):
    """20 000 generated Sequel reads (clamped dovetail ends, and ends spread with sigma = 100) at -c 3: the one-item build
    screens an H16 read on 32 lanes, the long-launch build on a 16-lane row — one table definition, so the same reads are
    deferred and the outputs are the same (and the oracle's)."""
    from yacrd_amd import host
    sflags = (host.SYNTH_F_JITTER | host.synth_f_sigma(sigma)) if sigma else 0
    o, iv, ln = host.synth_csr(host.SYNTH_SEQUEL, 20000, 2000000, 4400 + sigma, flags=sflags)
    n = np.diff(o.astype(np.int64))
    h16 = int(((n > 128) & (n <= 256)).sum())
    assert h16 > 15000, h16
    want = oracle.run(o, iv, ln.astype(np.uint64), 3, 0.4, n_threads=4)
    deferred = {}
    for flags in (ONE, TWO):
        with yacrd_amd.Engine(flags=flags) as e:
            assert_same(e.run(o, iv, ln, 3, 0.4), want, "sigma %d flags %d" % (sigma, flags))
            t = e.timing()
            assert t["screen_items"] == (2 if flags == TWO else 1), t
            deferred[flags] = t["deferred_reads"]
    print("sigma %d: deferred %d of %d reads (%d H16)" % (sigma, deferred[TWO], len(n), h16))
    assert deferred[ONE] == deferred[TWO], deferred
    assert 0 < deferred[TWO] < len(n) // 2, deferred  # the screen decides most reads and defers some
