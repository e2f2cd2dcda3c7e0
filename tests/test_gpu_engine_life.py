"""What an engine, a stream, a stream group and a gzip writer hold goes when they do.  The library counts the bytes of device
and pinned memory its owner types hold (yacrd_debug_live_bytes; csrc/engine_internal.h: DevBuf, PinBuf): every case reads the
count first, uses every kind of buffer on its way, closes what it made and finds the count where it was; what was computed on
the way is the oracle's."""
import os

import numpy as np
import pytest

import oracle
import yacrd_amd
from cases import assert_same, make_read
from yacrd_amd import host
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

CLS_GENERAL = 11  # csrc/device_common.h: reads beyond the workgroup classes' 16 384 intervals


def oracle_for(csr, cov=4, nc=0.4):
    return oracle.run(csr[0], csr[1], csr[2].astype(np.uint64), cov, nc, n_threads=4)


@pytest.fixture(scope="module")
def short():
    """300 reads, and the oracle's answer"""
    off, iv, ln = host.synth_csr(host.SYNTH_ONT, 300, 6000, 20260301)
    csr = (off, np.ascontiguousarray(iv).reshape(-1, 2), ln)
    return csr, oracle_for(csr)


@pytest.fixture(scope="module")
def with_huge(short):
    """the same with one read of 20 000 intervals behind them: the device-wide screen's, on the side stream"""
    (off, iv, ln), _ = short
    huge = make_read(np.random.default_rng(7), 20000, 800000)
    csr = (np.append(off, off[-1] + np.uint64(len(huge))), np.concatenate([iv, huge]), np.append(ln, np.uint32(800000)))
    return csr, oracle_for(csr)


@pytest.fixture(scope="module")
def pageable():
    """a batch whose intervals are more than 1 MiB of ordinary memory: it crosses through the engine's bounce buffers"""
    off, iv, ln = host.synth_csr(host.SYNTH_ONT, 2000, 100000, 20260302)
    csr = (off, np.ascontiguousarray(iv).reshape(-1, 2), ln)
    assert csr[1].nbytes > (1 << 20)
    return csr, oracle_for(csr)


def test_engine_with_a_device_wide_read_and_as_one_launch(short, with_huge):
    before = live_bytes()
    csr, want = with_huge
    with yacrd_amd.Engine(device_id=0) as e:
        assert_same(e.run(*csr, 4, 0.4), want, "with the huge read")
        assert e.debug_counters()["n"][CLS_GENERAL] == 1
        assert_same(e.run(*csr, 4, 0.4), want, "again (predicted)")
        assert live_bytes()[0] > before[0] and live_bytes()[1] > before[1]
    assert live_bytes() == before
    csr, want = short
    with yacrd_amd.Engine(device_id=0, flags=yacrd_amd.F_ONE_LAUNCH) as e:
        assert_same(e.run(*csr, 4, 0.4), want, "one launch")
        assert e.timing()["one_launch"] == 1
    assert live_bytes() == before


def test_submit_collect_device_forms_classify_and_bounce_buffers(short, pageable):
    import torch
    before = live_bytes()
    (off, iv, ln), want = short
    on_device = [torch.from_numpy(x).cuda() for x in (off.view(np.int64), iv.view(np.int32).reshape(-1), ln.view(np.int32))]
    torch.cuda.synchronize()
    assert live_bytes() == before  # (torch's memory is not the library's)
    with yacrd_amd.Engine(device_id=0) as e:
        e.submit(off, iv, ln, 4, 0.4)
        assert_same(e.collect(), want, "submit + collect")
        e.submit_device(*(t.data_ptr() for t in on_device), len(ln), int(off[-1]), 4, 0.4)
        assert e.wait().n_regions == len(want[1])
        assert_same(e.fetch(), want, "submit_device + wait")
        assert np.array_equal(e.classify(want[0], want[1], ln, 0.4), want[2])
        pinned_without_bounce = live_bytes()[1]
        assert_same(e.run(*pageable[0], 4, 0.4), pageable[1], "through the bounce buffers")
        assert live_bytes()[1] >= pinned_without_bounce + (4 << 20)
    assert live_bytes() == before


def test_stream_and_stream_group(golden_dir):
    before = live_bytes()
    path = os.path.join(golden_dir, "reads.paf")
    with open(os.path.join(golden_dir, "truth.yacrd")) as f:
        truth = set(l.rstrip("\n") for l in f)

    def report(c, got):
        return set(oracle.report_from_csr(c.names, c.lengths, got.bad_offsets, got.bad_regions, got.read_type))

    engines = [yacrd_amd.Engine(device_id=0) for _ in range(2)]
    try:
        with yacrd_amd.Stream(engines[0], 4096, 4) as s:
            c = host.ingest_stream(path, s.sink(), n_threads=2)
            assert report(c, s.finish(c.handle_map, c.lengths, 0, 0.8)) == truth
        with yacrd_amd.StreamGroup(engines, 4096, 4) as grp:
            c = host.ingest_stream(path, grp.sink(), n_threads=2)
            assert report(c, grp.finish(c.handle_map, c.lengths, 0, 0.8)) == truth
        with_engines = live_bytes()
        yacrd_amd.Stream(engines[0], 4096, 4).close()  # (nothing pushed)
        yacrd_amd.StreamGroup(engines, 4096, 4).close()
        assert live_bytes() == with_engines
    finally:
        for e in engines:
            e.close()
    assert live_bytes() == before


def test_gzip_writer_that_is_aborted(tmp_path):
    before = live_bytes()
    out = tmp_path / "never.gz"
    with yacrd_amd.Engine(device_id=0) as e:
        w = e.gzip_writer(str(out))
        w.write(b"ACGT" * 100000)
        assert live_bytes()[0] > before[0] and live_bytes()[1] > before[1]
        w.abort()
        assert not os.listdir(tmp_path)
        blob = e.gzip(b"ACGT" * 100000)  # (the engine has its encoder back)
        assert len(blob) > 28
    assert live_bytes() == before


def test_calls_that_fail_before_any_launch(short):
    before = live_bytes()
    (off, iv, ln), want = short
    with yacrd_amd.Engine(device_id=0) as e:
        with pytest.raises(yacrd_amd.EngineError, match="no result"):
            e.fetch()
        assert_same(e.run(off, iv, ln, 4, 0.4), want, "after a fetch of nothing")
        down = off.copy()
        down[1], down[2] = off[2], off[1]
        assert down[2] < down[1]
        with pytest.raises(yacrd_amd.EngineError, match="non-decreasing"):
            e.run(down, iv, ln, 4, 0.4)
        assert_same(e.run(off, iv, ln, 4, 0.4), want, "after offsets that go down")
        e.submit(off, iv, ln, 4, 0.4)
        with pytest.raises(yacrd_amd.EngineError, match="pending"):
            e.run(off, iv, ln, 4, 0.4)
        assert_same(e.collect(), want, "the batch that was pending")
        assert_same(e.run(off, iv, ln, 4, 0.4), want, "after a run under a pending batch")
    assert live_bytes() == before
