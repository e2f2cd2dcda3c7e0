"""The yardstick of the device report reader, pinned on the CPU: the Python restatement of the reader's rule
(tests/report_cases.py) equals yacrd_report_read on the seeded texts and on the golden report, and every corrupt case fails."""
import os

import pytest

import report_cases as rc
from yacrd_amd import host


def test_restatement_equals_the_host_reader_on_the_fuzz_set(tmp_path):
    sizes = set()
    for seed in range(500):
        text = rc.make_text(seed, rc.fuzz_sizes(seed))
        sizes.add(len(text))
        assert rc.same(rc.restate(text), rc.host_read(tmp_path, text)), "seed %d" % seed
    for k in (1, 2, 3):  # the set does reach the borders it claims
        assert any(abs(s - k * rc.TILE) <= 2 for s in sizes)
    assert any(abs(s - rc.CHUNK) <= 1 for s in sizes)


def test_restatement_equals_the_host_reader_on_the_golden_report(golden_dir):
    path = os.path.join(golden_dir, "truth.yacrd")
    with open(path, "rb") as f:
        want = rc.restate(f.read())
    assert len(want[0]) == 230
    assert rc.same(want, rc.host_read_file(path))


def test_replaced_rows_keep_their_position(tmp_path):
    text = b"x\ta\t10\t1,2,3\nx\tb\t20\t\nx\ta\t30\t\nx\t\t5\t9,8,7,6;,1,2\n"
    names, lengths, bo, br = rc.host_read(tmp_path, text)
    assert names == [b"a", b"b", b""] and lengths.tolist() == [30, 20, 5]
    assert bo.tolist() == [0, 0, 0, 2] and br.tolist() == [[8, 7], [1, 2]]
    assert rc.same(rc.restate(text), (names, lengths, bo, br))


@pytest.mark.parametrize("name", sorted(rc.CORRUPT))
def test_corrupt_cases_fail_in_the_host_reader(tmp_path, name):
    text = rc.corrupt_text(name)
    with pytest.raises(rc.Corrupt):
        rc.restate(text)
    with pytest.raises(host.HostError, match="seems corrupt at line 4"):
        rc.host_read(tmp_path, text)
