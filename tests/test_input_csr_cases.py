"""tests/input_csr_cases.py on the CPU: the comparison of two input CSRs reports every damaged interval that the comparison of
the sweep's output lets through, the reference for raw records agrees with the host parser's CSR, and the record generators
put their runs where they say.  The GPU half is tests/test_gpu_input_csr.py."""
import numpy as np
import pytest

import oracle
from yacrd_amd import host
from input_csr_cases import (BIG_READS, BIG_RECORDS, COUNT_EDGES, MUTATIONS, READ_COUNT_EDGES, UPLOAD_BYTES, assert_same_csr,
                             big_stream_case, csr_of_records, group_case, mutate, shuffled_inside_reads, stream_cases, upload_case)


@pytest.fixture(scope="module")
def batch():
    return host.synth_csr(host.SYNTH_ONT, 3000, 60000, 20241108)  # a pile-up of depth ~40: what the ingest tests sweep at -c 4


@pytest.mark.parametrize("kind", MUTATIONS)
def test_every_damaged_interval_is_reported(batch, kind):
    """One interval of one read damaged, 200 times per kind: assert_same_csr reports every one, and names the read.  (The same
    damage changes oracle.run's output at -c 4 for 0.6 % (end + 1) .. 33 % (another read's interval) of them: counted below.)"""
    rng = np.random.default_rng(MUTATIONS.index(kind))
    offsets, intervals, lengths = batch
    assert_same_csr(batch, batch, "the batch itself")
    want = oracle.run(offsets, intervals, lengths.astype(np.uint64), 4, 0.4, n_threads=4)
    seen_by_the_sweep = 0
    for k in rng.choice(len(intervals), 200, replace=False):
        bad = mutate(batch, kind, int(k), rng)
        r = int(np.searchsorted(offsets, np.uint64(k), side="right") - 1)
        with pytest.raises(AssertionError, match=r"read %d\b" % r):
            assert_same_csr(bad, batch, kind)
        if k % 4 == 0:  # (a quarter of them through the sweep: the figure, not a bound)
            a, b = int(bad[0][r]), int(bad[0][r + 1])
            one = oracle.run(np.array([0, b - a], np.uint64), bad[1][a:b], lengths[r:r + 1].astype(np.uint64), 4, 0.4, n_threads=1)
            w0, w1 = int(want[0][r]), int(want[0][r + 1])
            seen_by_the_sweep += not (np.array_equal(one[1], want[1][w0:w1]) and one[2][0] == want[2][r])
    print("%s: assert_same_csr reported 200 of 200; the sweep's output changed for %d of ~50" % (kind, seen_by_the_sweep))


def test_order_inside_a_read_matters_only_when_exact(batch):
    shuffled = shuffled_inside_reads(batch, np.random.default_rng(5))
    assert not np.array_equal(shuffled[1], batch[1])
    assert_same_csr(shuffled, batch, "shuffled inside reads")
    with pytest.raises(AssertionError, match="in value or order"):
        assert_same_csr(shuffled, batch, "shuffled inside reads", exact=True)
    assert_same_csr(batch, batch, "itself", exact=True)
    # rows that move BETWEEN reads are not a permutation inside reads
    moved = batch[1].copy()
    a, b = int(batch[0][10]), int(batch[0][20])
    moved[[a, b]] = moved[[b, a]]
    assert not np.array_equal(moved[a], moved[b])
    with pytest.raises(AssertionError, match=r"read 10\b"):
        assert_same_csr((batch[0], moved, batch[2]), batch, "swapped between reads")
    # lengths, counts, a missing CSR
    longer = batch[2].copy()
    longer[7] += 1
    with pytest.raises(AssertionError, match=r"length differs first at read 7\b"):
        assert_same_csr((batch[0], batch[1], longer), batch, "length")
    with pytest.raises(AssertionError, match="no input CSR"):
        assert_same_csr(None, batch, "none")
    with pytest.raises(AssertionError, match="reads, want"):
        assert_same_csr((batch[0][:-1], batch[1], batch[2][:-1]), batch, "a read short")


def test_the_reference_for_records_agrees_with_the_host_parser(tmp_path):
    from test_ingest_stream import PySink
    paf = str(tmp_path / "s.paf")
    host.synth_paf(host.SYNTH_ONT, 3000, 60000, 11, paf)
    ref = host.csr_from_file(paf, n_threads=2)
    sink = PySink(capacity=1000)
    c = host.ingest_stream(paf, sink.struct, n_threads=3)
    recs = sink.records()
    assert len(recs) == 60000 and c.names == ref.names
    off, iv = csr_of_records(recs, c.n_reads, c.handle_map)
    assert_same_csr((off, iv, c.lengths), (ref.offsets, ref.intervals, ref.lengths), "records of a synthetic PAF")
    # one engine's share of a group: the reads whose handle is k mod 3, in order
    inv = np.zeros(c.n_reads, np.int64)
    used = np.nonzero(c.handle_map != 0xFFFFFFFF)[0]
    inv[c.handle_map[used]] = used
    n = np.diff(ref.offsets.astype(np.int64))
    total = 0
    for k in range(3):
        keep = inv % 3 == k
        off_k, iv_k = csr_of_records(recs, c.n_reads, c.handle_map, keep)
        want_off = np.zeros(int(keep.sum()) + 1, np.uint64)
        want_off[1:] = np.cumsum(n[keep])
        assert_same_csr((off_k, iv_k, ref.lengths[keep]), (want_off, ref.intervals[np.repeat(keep, n)], ref.lengths[keep]), "share %d" % k)
        total += int(off_k[-1])
    assert total == int(ref.offsets[-1])


def test_the_generators_put_the_edges_where_they_say():
    cases = stream_cases()
    for n in COUNT_EDGES:
        assert len(cases["records_%d" % n][0]) == n
    for R in READ_COUNT_EDGES:
        recs, n_reads, _ = cases["reads_%d" % R]
        off, _ = csr_of_records(recs, n_reads)
        assert n_reads == R and off[R] > off[R - 1] and (np.diff(off.astype(np.int64)) == 0).sum() >= R - 10
    a = cases["run_head_on_lane_63"][0]["a"]
    assert a[62] != a[63] == a[64]
    a = cases["run_of_one_on_lane_63"][0]["a"]
    assert a[62] != a[63] != a[64] and (a[64:129] == a[64]).all() and a[129] != a[64]
    a = cases["run_of_64_from_lane_0"][0]["a"]
    assert (a[:64] == a[0]).all() and a[64] != a[0]
    a = cases["run_of_64_from_lane_1"][0]["a"]
    assert a[0] != a[1] and (a[1:65] == a[1]).all() and a[65] != a[1]
    a = cases["run_of_200_over_four_wavefronts"][0]["a"]
    assert a[99] != a[100] and (a[100:300] == a[100]).all() and a[300] != a[100] and 100 // 64 + 3 == 299 // 64 and 100 < 256 < 299
    a = cases["runs_of_one"][0]["a"]
    assert (a[1:] != a[:-1]).all()
    a = cases["alternating_ids"][0]["a"]
    assert (a[1:] != a[:-1]).all() and set(a.tolist()) == {0, 1}
    recs = cases["self_overlaps_inside_a_run"][0]
    assert 0 < (recs["a"] == recs["b"]).sum() < len(recs)
    recs, R, hmap = cases["map_many_handles_to_one_read"]
    assert len(hmap) > 10 * R and len(csr_of_records(recs, R, hmap)[0]) == R + 1
    recs, R, hmap = cases["map_permutes"]
    assert sorted(hmap.tolist()) == list(range(R)) and not np.array_equal(hmap, np.arange(R))
    recs, R, hmap = group_case()
    for N in (2, 3, 5):
        same = recs["a"] % N == recs["b"] % N
        assert same.sum() > 100 and (~same).sum() > 100 and (recs["a"] == recs["b"]).sum() > 100
    for case in cases.values():
        assert (case[0]["sa"] < case[0]["ea"]).all() and (case[0]["sb"] < case[0]["eb"]).all()
    assert [upload_case(b)[1].nbytes for b in UPLOAD_BYTES[:3]] == list(UPLOAD_BYTES[:3])
    off, iv, ln = upload_case(UPLOAD_BYTES[0])
    assert int(off[-1]) == len(iv) and len(ln) == len(off) - 1 and (np.diff(off.astype(np.int64))[:-1] == 100).all()


def test_the_large_case_is_past_both_thresholds():
    recs, R = big_stream_case()
    assert R == BIG_READS == 1025 * 4096 + 1 and len(recs) == BIG_RECORDS > 256 * 16 * 256
    a = recs["a"].astype(np.int64)
    assert (np.diff(a) >= 0).all() and (a[::10] == a[9::10]).all()
    off, iv = csr_of_records(recs, R)
    n = np.diff(off.astype(np.int64))
    assert n[0] and n[-1] and n[1024 * 4096 - 1] and n[1024 * 4096] and int(off[-1]) == 2 * BIG_RECORDS
    assert (n.reshape(-1)[:1025 * 4096].reshape(1025, 4096).sum(axis=1) > 0).all()  # every tile of the scan holds intervals
