"""The report's format as tests/report_write_cases.py restates it against the host writer (yacrd_report_write) on the CPU:
the yardstick tests/test_gpu_report_write.py measures the device writer with."""
import os

import numpy as np

import oracle
import report_write_cases as wc
from yacrd_amd import host


def test_restatement_equals_the_host_writer_on_300_seeded_tables(tmp_path):
    out = str(tmp_path / "w.yacrd")
    regions = 0
    for seed in range(300):
        t = wc.make_table(seed, tmp_path)
        regions += len(t.bad_regions)
        assert wc.host_write(out, t) == wc.restate(t), "seed %d" % seed
    assert regions > 3000  # (the maker does make regions)


def test_restatement_equals_the_host_writer_on_the_golden_table(golden_dir, tmp_path):
    c = host.csr_from_file(os.path.join(golden_dir, "reads.paf"), n_threads=2)
    bo, br, rt = oracle.run(c.offsets, c.intervals, c.lengths.astype(np.uint64), 0, 0.8)
    t = wc.Table([n.encode() for n in c.names], c.lengths, bo, np.asarray(br, np.uint32).reshape(-1, 2), rt)
    got = wc.host_write(str(tmp_path / "g.yacrd"), t)
    assert got == wc.restate(t)
    with open(os.path.join(golden_dir, "truth.yacrd"), "rb") as f:
        assert set(got.splitlines()) == set(f.read().splitlines()) and len(got.splitlines()) == 230


def test_restatement_equals_the_host_writer_on_the_edge_table(tmp_path):
    t = wc.edge_table()
    got = wc.host_write(str(tmp_path / "e.yacrd"), t)
    assert got == wc.restate(t)
    assert b"wraps\t1000\t4294966816,500,20;1,4294967295,0;4294967295,1,0\n" in got
    assert b"NotBad\tlen-0\t0\t\n" in got and b"\t\t5\t1,1,2\n" in got and b"\tno-region\t123456\t\n" in got
    assert b"4294967295,0,4294967295;0,4294967295,4294967295\n" in got


def test_a_type_beyond_2_is_an_error_of_the_host_writer(tmp_path):
    t = wc.table([b"a", b"b"], [1, 2], [[], []], [0, 3])
    try:
        wc.host_write(str(tmp_path / "bad.yacrd"), t)
    except host.HostError as x:
        assert "invalid read type" in str(x)
    else:
        raise AssertionError("a read type of 3 was written")
