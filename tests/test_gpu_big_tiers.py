"""Reads of more than 16 384 intervals, each tier of their cascade on its own edges: every case is the oracle's
bytes AND Engine.big_routes() — which of the four exact implementations decided the read.  The reads and their claims are
tests/big_cases.py's; tests/test_big_cases.py holds the claims against the CPU emulations."""
import functools

import numpy as np
import pytest

import big_cases as bc
import oracle
import yacrd_amd
from cases import assert_same, make_read

pytestmark = pytest.mark.gpu

FLAGS = {"default": 0, "no_prefilter": yacrd_amd.F_NO_PREFILTER, "force_general": yacrd_amd.F_FORCE_GENERAL}
assert FLAGS["no_prefilter"] == bc.F_NO_PREFILTER and FLAGS["force_general"] == bc.F_FORCE_GENERAL


@pytest.fixture(scope="module")
def engines():
    made = {name: yacrd_amd.Engine(device_id=0, flags=f) for name, f in FLAGS.items()}
    yield made
    for e in made.values():
        e.close()


def want_of(csr, c, threads=8):
    return oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), c, 0.4, n_threads=threads)


def summed(claims):
    return tuple(int(v) for v in np.sum(np.array(claims, dtype=np.int64).reshape(-1, 4), axis=0))


def check(e, csr, c, want, routes, ctx):
    assert_same(e.run(*csr, c, 0.4), want, ctx)
    assert e.big_routes() == tuple(routes), (ctx, e.big_routes(), routes)


@functools.lru_cache(maxsize=None)
def matrix_batch(ci):
    """the matrix at COVS[ci] with a read of 100 or 600 intervals after every eighth (the other classes' launches run beside the
    device-wide screen's side stream); the oracle's answer, computed once"""
    c, reads = bc.matrix(ci)
    rng = np.random.default_rng([4102, ci])
    batch, shapes = [], []
    for i, (shape, n, L, iv) in enumerate(reads):
        batch.append((iv, L))
        shapes.append((shape, n, L))
        if i % 8 == 7:
            batch.append((make_read(rng, (100, 600)[(i // 8) % 2], 50000, "regular"), 50000))
    csr = bc.csr_of(batch)
    return c, csr, want_of(csr, c), shapes


@pytest.mark.parametrize("ci", range(5))
def test_matrix_at_default_flags(ci):
    """every shape at every length it fits: the routes are the generators' claims summed, nothing is left unattributed; the same
    batch again on the same engine (launched on the first run's counts where those allow it): same bytes, same routes"""
    c, csr, want, shapes = matrix_batch(ci)
    routes = summed([bc.routes(shape, n, L, c) for shape, n, L in shapes])
    assert sum(routes) == len(shapes) and (routes[0] > 0) == (c <= 4) and routes[2] > 0 and routes[3] > 0
    with yacrd_amd.Engine(device_id=0) as e:
        for run in range(2):
            check(e, csr, c, want, routes, "matrix c %d run %d" % (c, run))


@pytest.mark.parametrize("ci", range(5))
@pytest.mark.parametrize("which", ("no_prefilter", "force_general"))
def test_matrix_without_the_front_tiers(engines, which, ci):
    c, csr, want, shapes = matrix_batch(ci)
    routes = summed([bc.routes(shape, n, L, c, FLAGS[which]) for shape, n, L in shapes])
    assert routes[0] == routes[1] == 0 and (routes[3] == len(shapes)) == (which == "force_general")
    assert routes[2] == (len(shapes) if which == "no_prefilter" else 0)
    check(engines[which], csr, c, want, routes, "matrix c %d %s" % (c, which))


@pytest.mark.parametrize("c", (0, 4))
def test_the_trim_cap(engines, c):
    """bt_plan_kernel's fits = m_new <= kBtCap, both sides: tests/test_big_cases.py::test_the_cap_edge_in_keys finds the comb that
    leaves exactly 16 384 keys (formulation.trim_keys is the kernel's m_new for plain reads: big_cases.trim_key_count says
    why): that read is swept in LDS, one interval more (16 386 keys; a kept set is balanced, 16 385 cannot be) takes the
    sort, whose scatter then reads cursor limits that hold nothing."""
    k = bc.cap_k(c)
    for kk, routes in ((k, (0, 1, 0, 0)), (k + 1, (0, 0, 1, 0))):
        csr = bc.csr_of([(bc.cap_read(c, kk), bc.CAP_L)])
        check(engines["default"], csr, c, want_of(csr, c, 1), routes, "cap c %d k %d" % (c, kk))
    both = bc.csr_of([(bc.cap_read(c, k + 1), bc.CAP_L), (bc.cap_read(c, k), bc.CAP_L), (bc.cap_read(c, k + 1), bc.CAP_L)])
    check(engines["default"], both, c, want_of(both, c, 2), (0, 1, 2, 0), "cap c %d, three reads" % c)


def test_more_than_1024_device_wide_reads():
    """bs_setup_kernel's second trip over the class list: 1100 reads of 5 and 6 chunks (16 385 / 20 481 intervals), so the chunk
    offset carried across read 1024 matters; the reads around the border and at both ends of the list are the ones the screen
    does not decide"""
    R, L, c = 1100, 5000, 4
    shape_at = {0: "holed", 1023: "holed", 1024: "holed", 1099: "holed", 1022: "comb", 1025: "comb"}
    batch, claims = [], []
    for r in range(R):
        n = (16385, 20481)[r % 2]
        shape = shape_at.get(r, "pile")
        batch.append((bc.SHAPES[shape](np.random.default_rng([4106, r]), n, L, c), L))
        claims.append(bc.routes(shape, n, L, c))
    assert summed(claims) == (1094, 4, 2, 0)
    csr = bc.csr_of(batch)
    want = want_of(csr, c)
    with yacrd_amd.Engine(device_id=0) as e:
        check(e, csr, c, want, (1094, 4, 2, 0), "1100 reads")


def test_a_read_of_more_than_2_to_the_20_intervals(engines):
    """big_scan_kernel's second trip over a read's chunks (P = 2^22 keys, 512 chunks of 8192), all three scans: the read whose
    257th chunk starts inside a region (tests/test_big_cases.py).  c = 2: in front of an even key index the depth is even."""
    c, L = bc.HUGE_C, bc.HUGE_L
    iv = bc.huge_sparse()
    assert len(iv) > 2**20
    front = bc.pile(np.random.default_rng([4107, 0]), bc.N_SMALL, 5000, c)
    back = bc.pile(np.random.default_rng([4107, 1]), bc.N_SMALL, 5000, c)
    csr = bc.csr_of([(front, 5000), (iv, L), (back, 5000)])
    want = want_of(csr, c, 1)
    assert int(want[0][2] - want[0][1]) > 10000  # regions of the long read: closings on both sides of every chunk border
    check(engines["no_prefilter"], csr, c, want, (0, 0, 3, 0), "2^20 intervals, no prefilter")
    assert engines["no_prefilter"].big_routes()[2] >= 1
    check(engines["default"], csr, c, want, (2, 0, 1, 0), "2^20 intervals")
    assert engines["default"].big_routes()[2] >= 1


@pytest.mark.parametrize("t", bc.ZL_T)
def test_two_zero_length_intervals_at_one_position(engines, t):
    """pass A's duplicate test with t keys in front of the pair: inside a thread's 32 keys, across a thread's first key, across a
    chunk's first key.  The read enters the sort ([2]) and leaves it for the exact kernel ([3]) with and without the front tiers
    (the comb's keys are too many for the trimming filter, so [1] stays 0)."""
    n, L, c = bc.N_CHUNKED, bc.CAP_L, 4
    csr = bc.csr_of([(bc.zl_pair_at(np.random.default_rng([4104, t]), n, L, c, t), L)])
    want = want_of(csr, c, 1)
    for which in ("no_prefilter", "default"):
        routes = bc.routes("zl_pair_at", n, L, c, FLAGS[which])
        assert routes == (0, 0, 1, 1)
        check(engines[which], csr, c, want, routes, "zl pair at %d, %s" % (t, which))


def test_a_missed_prediction_on_the_device_wide_reads():
    """A, A, B, B: B has A's reads and intervals but three reads beyond 16 384 intervals where A has two, so the device-wide screen
    launched on A's counts goes out a second time.  Each run's routes, and the reads the screens counted
    (YACRD_F_COUNT_PREFILTERED), are a fresh engine's on that batch: the final state, not both passes."""
    c, L = 4, 5000
    rng = np.random.default_rng(4108)
    small = [(make_read(rng, 600 + 100 * (i % 2), 50000, "regular"), 50000) for i in range(40)]
    a = [(bc.pile(rng, 20000, L, c), L), (bc.pile(rng, 17001, L, c), L), (bc.pile(rng, 12154, L, c), L)] + small
    b = [(bc.pile(rng, 16385, L, c), L), (bc.holed(rng, 16385, L, c), L), (bc.pile(rng, 16385, L, c), L)] + small
    a, b = bc.csr_of(a), bc.csr_of(b)
    assert len(a[2]) == len(b[2]) and int(a[0][-1]) == int(b[0][-1])
    wa, wb = want_of(a, c, 2), want_of(b, c, 2)
    fresh = {}
    for name, csr, want, routes in (("a", a, wa, (2, 0, 0, 0)), ("b", b, wb, (2, 1, 0, 0))):
        with yacrd_amd.Engine(device_id=0, flags=yacrd_amd.F_COUNT_PREFILTERED) as e:
            check(e, csr, c, want, routes, "fresh " + name)
            fresh[name] = (e.big_routes(), e.timing()["prefiltered_reads"])
    assert fresh["b"][1] >= 2
    with yacrd_amd.Engine(device_id=0, flags=yacrd_amd.F_COUNT_PREFILTERED) as e:
        seen = []
        for i, (name, csr, want) in enumerate((("a", a, wa), ("a", a, wa), ("b", b, wb), ("b", b, wb))):
            check(e, csr, c, want, fresh[name][0], "run %d" % i)
            t = e.timing()
            seen.append((t["predicted"], t["prediction_misses"]))
            assert t["prefiltered_reads"] == fresh[name][1], (i, t["prefiltered_reads"], fresh[name][1])
        assert seen[1] == (1, 0) and seen[2][1] == 1, seen  # A again: predicted; B on A's counts: a miss
