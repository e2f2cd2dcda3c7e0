"""The input CSR itself — in_off / in_iv / in_len as the sweeps read them — where the GPU builds or stages it: the streaming
build (csrc/csr_build.h: count, scan, scatter), one stream and a group; the device parser (csrc/gpu_paf.hip), one engine and
several; the upload of yacrd_engine_run (yke::h2d).  Engine.debug_input_csr brings it home and every case compares it with
numpy (tests/input_csr_cases.py: csr_of_records) or with the oracle's ingest, interval by interval: the sweep's output, which
the other ingest tests compare, hardly moves when one interval of a pile-up is wrong (tests/test_input_csr_cases.py)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
import yacrd_amd
from yacrd_amd import host
from cases import assert_same
from coordinate_cases import edge_text
from input_csr_cases import (READ_LENGTH, UPLOAD_BYTES, assert_same_csr, assert_same_csr_in_ranges, big_stream_case, csr_of_records,
                             group_case, handle_of_read, stream_cases, upload_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def engines():
    es = [yacrd_amd.Engine() for _ in range(5)]
    yield es
    for e in es:
        e.close()


# ---- the streaming build, raw records ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream(engine):
    with yacrd_amd.Stream(engine, 4096, 4) as st:  # (every small case is one buffer: record i sits on lane i % 64)
        yield st


@pytest.mark.parametrize("name", sorted(stream_cases()))
def test_streaming_build(engine, stream, name):
    recs, n_reads, handle_map = stream_cases()[name]
    lengths = np.full(n_reads, READ_LENGTH, np.uint32)
    offsets, intervals = csr_of_records(recs, n_reads, handle_map)
    stream.push(recs)
    got = stream.finish(handle_map, lengths, 0, 0.8)
    assert stream.stats()["n_records"] == len(recs)
    assert_same_csr(engine.debug_input_csr(), (offsets, intervals, lengths), name)
    assert_same(got, oracle.run(offsets, intervals, lengths.astype(np.uint64), 0, 0.8, n_threads=2), name)


def test_streaming_build_past_one_grid_and_1024_scan_tiles(engine):
    """4 198 401 reads (1025 tiles of the scan and one read: scan_parts_kernel's carry loop takes a second trip) and 1.15 M
    records (more than 256 * 16 records per CU: both grid-stride loops of the count and the scatter take a second trip)."""
    recs, n_reads = big_stream_case()
    lengths = np.full(n_reads, READ_LENGTH, np.uint32)
    want = csr_of_records(recs, n_reads) + (lengths,)
    t0 = time.perf_counter()
    with yacrd_amd.Stream(engine, 131072, 4) as st:
        st.push(recs)
        st.finish(None, lengths, 0, 0.8)
        t1 = time.perf_counter()
        got = engine.debug_input_csr()
    t2 = time.perf_counter()
    assert_same_csr(got, want, "the large case")
    print("large case: push + finish %.2f s, the CSR home %.2f s, compared in %.2f s" % (t1 - t0, t2 - t1, time.perf_counter() - t2))


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_stream_group_engines_hold_their_share(engines, n):
    recs, n_reads, handle_map = group_case()
    lengths = (READ_LENGTH + np.arange(n_reads)).astype(np.uint32)  # (all different: a read's length must follow it to its engine)
    with yacrd_amd.StreamGroup(engines[:n], 999, 4) as grp:
        grp.push(recs)
        got = grp.finish(handle_map, lengths, 0, 0.8)
        owner = np.array([yacrd_amd.stream_device_of(h, n) for h in handle_of_read(handle_map, n_reads)])
        rec_owner = [np.array([yacrd_amd.stream_device_of(h, n) for h in recs[side]]) for side in "ab"]
        held = 0
        for k in range(n):
            csr = engines[k].debug_input_csr()
            offsets, intervals = csr_of_records(recs, n_reads, handle_map, owner == k)
            assert_same_csr(csr, (offsets, intervals, lengths[owner == k]), "%d engines, engine %d" % (n, k))
            # its share: the halves that name its reads, those of self-overlaps both; the other halves are nowhere
            assert len(csr[1]) == int((rec_owner[0] == k).sum() + (rec_owner[1] == k).sum())
            held += len(csr[1])
        assert held == 2 * len(recs)
    offsets, intervals = csr_of_records(recs, n_reads, handle_map)
    assert_same(got, oracle.run(offsets, intervals, lengths.astype(np.uint64), 0, 0.8, n_threads=2), "%d engines" % n)


# ---- the device parser, one engine: the build that trusts the parser's counts -----------------------------------------------
def _parsed(engine, text, fmt, ctx):
    engine.ingest_text(text.encode("utf-8"), 0, 0.8, fmt=fmt)
    names, offsets, intervals, lengths = oracle.to_csr((oracle.parse_m4 if fmt == 2 else oracle.parse_paf)(text))
    assert_same_csr(engine.debug_input_csr(), (offsets, intervals, lengths), ctx)


def test_parser_fixture_paf_and_m4(engine, golden_dir):
    from test_gpu_ingest import _paf_to_m4
    with open(os.path.join(golden_dir, "reads.paf"), newline="") as f:
        text = f.read()
    _parsed(engine, text, 1, "reads.paf")
    _parsed(engine, _paf_to_m4(text), 2, "reads.paf as M4")


def test_parser_random_plain_texts(engine):
    from test_gpu_ingest import _random_paf
    rng = np.random.default_rng(20260102)
    for case in range(200):
        _parsed(engine, _random_paf(rng, int(rng.integers(0, 120)), 0), 1, "random text %d" % case)


def test_parser_long_lines_across_tiles(engine):
    from test_gpu_ingest import _long_line_texts
    for crlf, text in _long_line_texts():
        _parsed(engine, text, 1, "long lines, %s" % ("CRLF" if crlf else "LF"))


@pytest.mark.parametrize("m4", [False, True])
def test_parser_coordinates_up_to_u32(engine, m4):
    """a wrong digit of a coordinate near 2^32 is invisible to the sweep: such a read goes to the exact path either way"""
    _parsed(engine, edge_text(m4), 2 if m4 else 1, "edge text, %s" % ("M4" if m4 else "PAF"))


# ---- the device parser, several engines -------------------------------------------------------------------------------------
def test_parser_group_lines_at_the_range_boundaries(engines, tmp_path):
    from test_gpu_ingest_group import BOUNDARY_SHAPES, _boundary_case
    for shape in BOUNDARY_SHAPES:
        text, names, offsets, intervals, lengths = _boundary_case(shape)
        raw = text.encode("utf-8")
        for n in (2, 3, 5):
            got = yacrd_amd.ingest_overlaps(engines[:n], raw, 0, 0.8)
            assert got[1] == list(names)
            assert_same_csr_in_ranges([e.debug_input_csr() for e in engines[:n]], (offsets, intervals, lengths), "%s, %d engines" % (shape, n))


_GROUP_WORKER = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import yacrd_amd
from yacrd_amd.engine import peer_copy_counts
from input_csr_cases import assert_same_csr_in_ranges
paf, route = sys.argv[2], sys.argv[4]
want = np.load(sys.argv[3])
want = (want["offsets"], want["intervals"], want["lengths"])
es = [yacrd_amd.Engine() for _ in range(5)]
for n in (2, 3, 5):
    before = peer_copy_counts()
    got = yacrd_amd.ingest_overlaps(es[:n], paf, 0, 0.8)
    moved = [a - b for a, b in zip(peer_copy_counts(), before)]
    # (the text was cut into ranges: the engines copied lengths, counts and, on a forced route, records to one another)
    assert moved[{"none": 0, "peer": 1, "staged": 2}[route]] > 0 and sum(moved) == max(moved), (n, moved)
    assert got[3]["n_reads"] == len(want[2]) and 2 * got[3]["n_records"] == int(want[0][-1])
    assert_same_csr_in_ranges([e.debug_input_csr() for e in es[:n]], want, "%d engines, route %s" % (n, route))
print("GROUP_WORKER OK")
"""


@pytest.fixture(scope="module")
def synthetic_paf(tmp_path_factory):
    d = tmp_path_factory.mktemp("input_csr")
    paf = str(d / "s.paf")
    host.synth_paf(host.SYNTH_ONT, 3000, 60000, 21, paf)
    with open(paf, newline="") as f:
        names, offsets, intervals, lengths = oracle.to_csr(oracle.parse_paf(f.read()))
    np.savez(str(d / "want.npz"), offsets=offsets, intervals=intervals, lengths=lengths)
    return paf, str(d / "want.npz")


@pytest.mark.parametrize("route", ["none", "peer", "staged"])
def test_parser_group_engines_hold_their_ranges(synthetic_paf, tmp_path, route):
    """2, 3 and 5 engines on one device over a synthetic PAF (ONT, 3000 reads / 60000 overlaps, 4.4 MB), the ranges cut every
    256 KiB so that every engine parses one; reading the other engines' records in place, and with every cross-engine copy
    forced through hipMemcpyPeerAsync / the host-staged route.  Both switches are read once per process: a child each."""
    paf, want = synthetic_paf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "group_worker.py"
    script.write_text(_GROUP_WORKER)
    env = dict(os.environ, YACRD_TEST_RANGE_BYTES="262144")
    env.pop("YACRD_TEST_FORCE_PEER_COPY", None)
    if route != "none":
        env["YACRD_TEST_FORCE_PEER_COPY"] = route
    p = subprocess.run([sys.executable, str(script), root, paf, want, route], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert p.stdout.splitlines()[-1] == "GROUP_WORKER OK", p.stdout[-2000:]


# ---- the upload of yacrd_engine_run -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bytes", UPLOAD_BYTES)
def test_upload_returns_the_arrays_bit_for_bit(engine, n_bytes):
    """pageable arrays cross in 4 MiB pieces through 12 pinned buffers filled by copy threads (13 pieces and 8 bytes: every
    buffer is refilled); pinned ones by direct DMA"""
    csr = upload_case(n_bytes)
    assert csr[1].nbytes == n_bytes
    engine.run(*csr, 0, 0.8)
    assert_same_csr(engine.debug_input_csr(), csr, "pageable, %d bytes" % n_bytes, exact=True)
    pinned = [yacrd_amd.PinnedArray.copy_of(x) for x in csr]
    try:
        engine.run(*(p.array for p in pinned), 0, 0.8)
        assert_same_csr(engine.debug_input_csr(), csr, "pinned, %d bytes" % n_bytes, exact=True)
    finally:
        for p in pinned:
            p.close()


# ---- the hook's own contract ------------------------------------------------------------------------------------------------
def test_the_hook_answers_only_for_the_engines_own_input(golden_dir):
    import torch
    csr = host.synth_csr(host.SYNTH_ONT, 50, 700, 3)
    other = host.synth_csr(host.SYNTH_ONT, 20, 300, 4)
    on_device = [torch.from_numpy(x).cuda() for x in (other[0].view(np.int64), other[1].view(np.int32).reshape(-1), other[2].view(np.int32))]
    torch.cuda.synchronize()
    with yacrd_amd.Engine() as e:
        assert e.debug_input_csr() is None                       # a fresh engine
        e.run(*csr, 0, 0.8)
        assert_same_csr(e.debug_input_csr(), csr, "run", exact=True)
        e.run_device(*(t.data_ptr() for t in on_device), len(other[2]), int(other[0][-1]), 0, 0.8)
        assert e.debug_input_csr() is None                       # somebody else's pointers were swept
        e.run(*other, 0, 0.8)
        assert_same_csr(e.debug_input_csr(), other, "run after run_device", exact=True)
        e.ingest_report(os.path.join(golden_dir, "truth.yacrd"), 0.8)
        assert e.debug_input_csr() is None                       # in_len holds a report's lengths now
        e.run(*csr, 0, 0.8)
        assert_same_csr(e.debug_input_csr(), csr, "run after ingest_report", exact=True)
        e.trim()
        assert e.debug_input_csr() is None
        e.submit(*other, 0, 0.8)
        assert e.debug_input_csr() is None                       # a submitted batch is pending
        e.collect()
        assert_same_csr(e.debug_input_csr(), other, "submit + collect", exact=True)
        with yacrd_amd.Stream(e, 64, 2) as st:                   # a failed call leaves none
            bad = np.zeros(3, dtype=yacrd_amd.OVL_REC_DTYPE)
            bad["b"][1] = 99
            st.push(bad)
            with pytest.raises(yacrd_amd.EngineError, match="outside"):
                st.finish(None, csr[2], 0, 0.8)
            assert e.debug_input_csr() is None
        e.run(np.zeros(1, np.uint64), np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32), 0, 0.8)  # no reads at all
        off, iv, ln = e.debug_input_csr()
        assert off.tolist() == [0] and iv.shape == (0, 2) and ln.shape == (0,)
