"""HIP path vs CPU oracle over the whole u32 coordinate range and on the edge of the event keys' range (kMaxKeyPos =
0x3FFFFFFE, csrc/device_common.h): every kernel family's guard and bin geometry, bit-exact through the C ABI.  The batches are
tests/coordinate_cases.py's; tests/test_coordinates.py proves the oracle at these coordinates and asserts, without a GPU, that
the batches hold what they are meant to hold.  Needs an MI355X."""
import numpy as np
import pytest

import oracle
import yacrd_amd
import coordinate_cases as cc
from cases import assert_same
from coordinate_cases import K
from yacrd_amd import (F_ALWAYS_DEFER, F_COUNT_PREFILTERED, F_FORCE_GENERAL, F_FORCE_LDS_SORT, F_NO_DEFER, F_NO_FUSED_SCREEN,
                       F_NO_HALVES, F_NO_PREFILTER, F_ONE_LAUNCH, F_SCREEN_ITEMS_2, F_SCREEN_WIDE, F_STREAM_SCREEN, F_WAVE_ONLY)

pytestmark = pytest.mark.gpu

COVERAGES = (0, 4, 5, 0xFFFFFFFF)
REGISTER_FLAGS = (F_ALWAYS_DEFER, F_NO_DEFER, F_NO_PREFILTER, F_ALWAYS_DEFER | F_SCREEN_ITEMS_2, F_ALWAYS_DEFER | F_SCREEN_WIDE,
                  F_ONE_LAUNCH)
WORKGROUP_FLAGS = (0, F_NO_PREFILTER, F_NO_FUSED_SCREEN, F_STREAM_SCREEN)
DEVICE_WIDE_FLAGS = (0, F_NO_PREFILTER)
SCREENING = {F_ALWAYS_DEFER, F_ALWAYS_DEFER | F_SCREEN_ITEMS_2, F_ALWAYS_DEFER | F_SCREEN_WIDE, F_ONE_LAUNCH}  # register builds with the screen


def _want(csr, cov):
    return oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), cov, 0.4, n_threads=8)


# ---- the screens' crafted edges at lengths 2^20 - 1 .. 2^32 - 1 ------------------------------------------------------------
def _screen_sweep(which, flag_sets, screening, cov):
    """The whole batch against the oracle under every flag set; then the reads the fast paths may keep (length <= K) alone, to
    see on the counters that the screen decided some of them and, in the deferring build, left some to the sort."""
    csr = cc.screen_batch(which)
    small = cc.sub_batch(csr, csr[2] <= K)
    want, want_small = _want(csr, cov), _want(small, cov)
    for flags in flag_sets:
        with yacrd_amd.Engine(flags=flags | F_COUNT_PREFILTERED) as e:
            assert_same(e.run(*csr, cov, 0.4), want, "%s cov %d flags %d" % (which, cov, flags))
            assert_same(e.run(*small, cov, 0.4), want_small, "%s cov %d flags %d, lengths <= K" % (which, cov, flags))
            t = e.timing()
            print("%s cov %d flags %d: prefiltered %d deferred %d of %d" % (which, cov, flags, t["prefiltered_reads"],
                                                                           t["deferred_reads"], len(small[2])))
            if cov <= 5 and flags in screening:
                assert t["prefiltered_reads"] > 0, (which, cov, flags)
            if cov <= 5 and flags == F_ALWAYS_DEFER:
                assert t["deferred_reads"] > 0, (which, cov, flags)


@pytest.mark.parametrize("cov", COVERAGES)
def test_register_screen_length_sweep(cov):
    """screen_reg.h, finish_compact.h, sweep_wave.h, one_batch.h: reads of 65 .. 256 intervals at 41 lengths"""
    _screen_sweep("register", REGISTER_FLAGS, SCREENING, cov)


@pytest.mark.parametrize("cov", COVERAGES)
def test_workgroup_screen_length_sweep(cov):
    """screen_wg.h, screen_stream.h, sweep_filtered.h, sweep_lds.h: reads of 513, 4097 and 16 384 intervals at every third length"""
    _screen_sweep("workgroup", WORKGROUP_FLAGS, {0, F_NO_FUSED_SCREEN, F_STREAM_SCREEN}, cov)


@pytest.mark.parametrize("cov", COVERAGES)
def test_device_wide_screen_length_sweep(cov):
    """screen_big.h, sweep_big_trim.h, sweep_big.h: test_device_wide_screen_edges' reads of 16 385 intervals at five lengths"""
    _screen_sweep("device_wide", DEVICE_WIDE_FLAGS, {0}, cov)


# ---- random batches of every size class, scaled ----------------------------------------------------------------------------
ENGINE_FLAGS = (0, F_FORCE_GENERAL, F_FORCE_LDS_SORT, F_WAVE_ONLY, F_NO_HALVES, F_ONE_LAUNCH)


@pytest.fixture(scope="module")
def engines():
    engs = [yacrd_amd.Engine(flags=f) for f in ENGINE_FLAGS]
    yield engs
    for e in engs:
        e.close()


def _through_device_pointers(e, csr, cov):
    import torch
    o, iv, ln = csr
    t = [torch.from_numpy(x).cuda() for x in (o.view(np.int64), np.ascontiguousarray(iv).view(np.int32).reshape(-1), ln.view(np.int32))]
    torch.cuda.synchronize()
    out = e.run_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(ln), int(o[-1]), cov, 0.4)
    got = e.fetch()
    assert int(out.n_regions) == int(got.bad_offsets[-1])
    return got


def _scaled_class_batches(size, runs):
    """One batch of reads of `size` intervals per goal, at k = 1 and scaled so that the largest length lands on K, K + 1, 2^31
    and next to 2^32 - 1: each against the oracle, and the scaled one against k times the engine's own k = 1 regions (a
    difference there is a coordinate bug, whatever the oracle says)."""
    for goal in cc.GOALS:
        csr, k = cc.class_batch(size, goal)
        big = cc.scaled(csr, k)
        for cov in (0, 1, 4):
            want1, wantk = _want(csr, cov), _want(big, cov)
            for run, name in runs:
                ctx = "size %d goal %s cov %d %s" % (size, goal, cov, name)
                got1, gotk = run(csr, cov), run(big, cov)
                own = (got1.bad_offsets, (got1.bad_regions.astype(np.uint64) * np.uint64(k)).astype(np.uint32), got1.read_type)
                assert int(got1.bad_regions.max(initial=0)) * k <= cc.U32
                assert_same(gotk, own, ctx + ": k x its own k = 1 regions")
                assert_same(got1, want1, ctx + ", k = 1")
                assert_same(gotk, wantk, ctx + ", k = %d" % k)


@pytest.mark.parametrize("size", cc.CLASS_SIZES)
def test_scaled_class_batches(engines, size):
    """the sorts of every class and the exact path: default, F_FORCE_GENERAL, F_FORCE_LDS_SORT, F_WAVE_ONLY, F_NO_HALVES, F_ONE_LAUNCH"""
    _scaled_class_batches(size, [(lambda csr, cov, e=e: e.run(*csr, cov, 0.4), "flags %d" % f) for e, f in zip(engines, ENGINE_FLAGS)])


@pytest.mark.parametrize("size", cc.CLASS_SIZES)
def test_scaled_class_batches_through_device_pointers(engines, size):
    """the same batches from device memory: run_device + fetch on the default engine"""
    _scaled_class_batches(size, [(lambda csr, cov: _through_device_pointers(engines[0], csr, cov), "run_device + fetch")])


# ---- one interval on the edge of the key range, the neighbours plain -------------------------------------------------------
EDGE_FLAGS = (0, F_FORCE_GENERAL, F_FORCE_LDS_SORT, F_WAVE_ONLY, F_NO_HALVES) + REGISTER_FLAGS + WORKGROUP_FLAGS[2:]


@pytest.mark.parametrize("n", cc.EDGE_SIZES)
def test_one_interval_on_the_edge(n):
    """Reads of n plain intervals with one replaced by (E - 5, E), (E, E), (E, E - 5), (0, E) for E on either side of K, 2^31
    and at 2^32 - 1, in every slot of a shared wavefront, beside untouched reads: the whole batch bit-exact, so a read its
    wavefront hands to the exact path must not disturb its neighbours.  Every build that owns a guard."""
    csr = cc.edge_batch(n)
    for cov in (0, 4):
        want = _want(csr, cov)
        for flags in EDGE_FLAGS:
            with yacrd_amd.Engine(flags=flags) as e:
                assert_same(e.run(*csr, cov, 0.4), want, "n %d cov %d flags %d" % (n, cov, flags))


# ---- the same edge through the text path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m4", [False, True])
def test_edge_text_through_the_device_parser(tmp_path, m4):
    """Lengths 4294967295, K and K + 1, part 4's coordinates: the device parser against the host parser and the oracle's
    ingest, the regions against the oracle, the resident report against the format restated."""
    import report_write_cases as wc
    from yacrd_amd import host
    fmt = 2 if m4 else 1
    path = str(tmp_path / ("edge.m4" if m4 else "edge.paf"))
    with open(path, "w", newline="") as f:
        f.write(cc.edge_text(m4))
    reads = (oracle.parse_m4 if m4 else oracle.parse_paf)(cc.edge_text(m4))
    w_names, off, iv, ln = oracle.to_csr(reads)
    c = host.csr_from_file(path, fmt=fmt, n_threads=2)
    assert c.names == list(w_names) and np.array_equal(c.lengths.astype(np.uint64), ln)
    assert np.array_equal(c.offsets, off) and np.array_equal(c.intervals, iv)
    for cov in (0, 1, 4):
        want = oracle.run(off, iv, ln, cov, 0.4, n_threads=2)
        with yacrd_amd.Engine() as e:
            got, names, lengths, stats = e.ingest_paf(path, cov, 0.4, fmt=fmt)
            assert names == list(w_names) and np.array_equal(lengths.astype(np.uint64), ln)
            assert stats["n_reads"] == 3 and stats["n_records"] * 2 == int(off[-1])
            assert_same(got, want, "%s cov %d" % (path, cov))
            table = wc.Table([s.encode() for s in names], lengths, want[0], want[1], want[2])
            assert e.report_text() == wc.restate(table)
            assert e.report_write_stats["resident"] == 1
