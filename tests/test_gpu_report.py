"""The device report reader (csrc/gpu_report.hip: yacrd_engine_ingest_report / _mem, Engine.ingest_report) against the
host reader (yacrd_report_read + Engine.classify): names, lengths, offsets, regions and types bit for bit; what must fall
back does, leaves nothing and leaves the engine usable; the CLI writes the same bytes down either path."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import report_cases as rc
import yacrd_amd
from yacrd_amd import host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
SEG = 32 * rc.CHUNK  # what the mover hands on at once (csrc/gpu_text.h: kTextSeg chunks)


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


def device_read(e, src, n=0.4):
    res, names, lengths, stats = e.ingest_report(src, n)
    got = ([s.encode("utf-8", "surrogateescape") for s in names], lengths, res.bad_offsets, res.bad_regions)
    return got, res.read_type, stats


def check(e, text, want, n=0.4, path=None):
    """the device's arrays for `text` (or the file at `path`) equal `want` and the types equal Engine.classify's"""
    got, types, stats = device_read(e, text if path is None else path, n)
    assert rc.same(got, want)
    assert stats["n_reads"] == len(want[0])
    R = len(want[0])
    ref = e.classify(want[2], want[3], want[1], n) if R else np.zeros(0, np.uint8)
    assert types.dtype == np.uint8 and np.array_equal(types, ref)
    return stats


@pytest.mark.parametrize("n", [0.2, 0.4, 0.8])
def test_golden_report(engine, golden_dir, n):
    path = os.path.join(golden_dir, "truth.yacrd")
    want = rc.host_read_file(path)
    stats = check(engine, None, want, n, path=path)
    assert stats["n_records"] == 230 and stats["text_bytes"] == os.path.getsize(path)
    with open(path, "rb") as f:
        check(engine, f.read(), want, n)


def test_fuzz_set_equals_the_host_reader_without_a_fallback(engine, tmp_path):
    for seed in range(300):
        text = rc.make_text(seed, rc.fuzz_sizes(seed))
        want = rc.host_read(tmp_path, text)  # (the host reader alone accepts all of them: it raises otherwise)
        try:
            check(engine, text, want, (0.2, 0.4, 0.8)[seed % 3])
        except yacrd_amd.NeedsHostParser as x:
            pytest.fail("seed %d fell back: %s" % (seed, x))
        except AssertionError:
            raise AssertionError("seed %d differs from the host reader" % seed)


def test_duplicates_keep_the_first_position_and_the_last_values(engine, tmp_path):
    rows = [b"NotBad\tr%d\t%d\t1,0,%d\n" % (i, 1000 + i, i + 1) for i in range(6000)]
    rows[0] = b"Chimeric\tdup\t11\t1,2,3;4,5,6\n"
    rows[4999] = b"NotBad\tdup\t22\t\n"
    rows[-1] = b"NotCovered\tdup\t33\t7,8,9"  # the last line, without a newline
    text = b"".join(rows)
    want = rc.host_read(tmp_path, text)
    assert want[0][0] == b"dup" and want[1][0] == 33 and want[3][0].tolist() == [8, 9] and len(want[0]) == 5998
    check(engine, text, want)


def test_two_alternating_ids_under_contention(engine, tmp_path):
    text = b"".join(b"x\t%s\t%d\t%d,%d,%d\n" % (b"ab"[i & 1:(i & 1) + 1] * 3, i + 1, i, i, i + 5) for i in range(60000))
    want = rc.host_read(tmp_path, text)
    assert want[0] == [b"aaa", b"bbb"] and want[1].tolist() == [59999, 60000] and want[3].tolist() == [[59998, 60003], [59999, 60004]]
    check(engine, text, want)


def _straddle(border):
    """a text whose row of 30 regions begins ~200 bytes in front of `border` and ends behind it"""
    head = rc.make_text(4242, border - 200)
    if not head.endswith(b"\n"):
        head += b"\n"
    body = b";".join(b"%d,%d,%d" % (k, 100 * k, 100 * k + 50) for k in range(30))
    assert len(body) > 250
    return head + b"NotBad\tstraddler\t5000\t" + body + b"\n" + rc.GOOD_ROW * 3


@pytest.mark.parametrize("border", [rc.TILE, 2 * rc.TILE, rc.CHUNK], ids=["tile", "two_tiles", "chunk"])
def test_a_row_straddles_a_border(engine, tmp_path, border):
    text = _straddle(border)
    want = rc.host_read(tmp_path, text)
    assert b"straddler" in want[0]
    check(engine, text, want)


def test_one_row_with_100000_regions(engine, tmp_path):
    body = b";".join(b"%d,%d,%d" % (k, 3 * k, 3 * k + 2) for k in range(100000))
    assert len(body) > 5 * rc.TILE
    text = rc.GOOD_ROW + b"Chimeric\tlong\t4000000000\t" + body + b"\r\n" + rc.GOOD_ROW.replace(b"read-ok", b"behind")
    want = rc.host_read(tmp_path, text)
    assert int(want[2][2] - want[2][1]) == 100000
    check(engine, text, want)


@pytest.mark.parametrize("text", [b"", b"\n", b"\n\r\n\n\r\n" * 9000, b"\r"], ids=["empty", "newline", "blank_lines", "cr"])
def test_no_lines_give_no_reads(engine, tmp_path, text):
    want = rc.host_read(tmp_path, text)
    assert want[0] == []
    stats = check(engine, text, want)
    assert stats["n_records"] == 0
    path = tmp_path / "blank.yacrd"
    path.write_bytes(text)
    check(engine, None, want, path=str(path))


def test_one_line_without_a_newline(engine, tmp_path):
    text = b"NotCovered\tonly\t77\t3,0,3;9,70,77"
    want = rc.host_read(tmp_path, text)
    assert want[0] == [b"only"] and want[3].tolist() == [[0, 3], [70, 77]]
    check(engine, text, want)


def _big_report(R):
    ids = np.arange(R)
    rows = np.char.add(np.char.add(np.char.add("NotBad\tread/", ids.astype(str)), "\t"), (ids % 50000 + 100).astype(str))
    rows = np.char.add(rows, np.where(ids % 3 == 0, "\t", np.char.add(np.char.add("\t7,0,", (ids % 90 + 1).astype(str)), ";2,50,60")))
    return ("\n".join(rows.tolist()) + "\n").encode()


def test_200000_reads_file_and_memory_warm_and_after_trim(engine, tmp_path):
    text = _big_report(200000)
    path = tmp_path / "big.yacrd"
    path.write_bytes(text)
    want = rc.host_read_file(str(path))
    assert len(want[0]) == 200000
    first, types, _ = device_read(engine, str(path))
    assert rc.same(first, want)
    assert np.array_equal(types, engine.classify(want[2], want[3], want[1], 0.4))
    for src in (text, str(path)):  # the memory form, then the file form again into warm buffers
        got, t2, _ = device_read(engine, src)
        assert rc.same(got, want) and np.array_equal(t2, types)
    engine.trim()
    got, t3, _ = device_read(engine, text)
    assert rc.same(got, want) and np.array_equal(t3, types)


@pytest.mark.parametrize("name", sorted(rc.CORRUPT))
def test_corrupt_reports_fall_back_and_leave_the_engine_usable(engine, tmp_path, name):
    text = rc.corrupt_text(name)
    with pytest.raises(host.HostError):
        rc.host_read(tmp_path, text)
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.ingest_report(text, 0.4)
    path = tmp_path / "bad.yacrd"
    path.write_bytes(text)
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.ingest_report(str(path), 0.4)
    good = rc.GOOD_ROW * 4
    check(engine, good, rc.host_read(tmp_path, good))  # the next call


def test_c_abi_returns_nothing_on_fallback(engine):
    import ctypes
    from yacrd_amd import engine as eng
    lib = yacrd_amd.load_library()
    res, rd, st = eng._Result(), eng._Reads(), eng._IngestStats()
    text = rc.corrupt_text("one_comma")
    buf = ctypes.create_string_buffer(text, len(text))
    rcode = lib.yacrd_engine_ingest_report_mem(engine._h, ctypes.addressof(buf), len(text), 0, 0.4, ctypes.byref(res), ctypes.byref(rd),
                                               ctypes.byref(st))
    assert rcode == eng.E_FALLBACK
    assert not res.bad_offsets and not res.bad_regions and not res.read_type and res.n_reads == 0
    assert not rd.lengths and not rd.name_off and not rd.names and rd.n_reads == 0


def test_a_bad_line_behind_the_first_segment_falls_back(engine):
    row = b"NotBad\tsame-read-again-and-again\t1000\t12,0,12;5,995,1000;1,2,3;4,5,6;7,8,9\n"
    text = row * (SEG // len(row) + 1000) + rc.CORRUPT["trailing_semicolon"] + row * 10
    assert len(text) > SEG + 4096
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.ingest_report(text, 0.4)
    good = text.replace(rc.CORRUPT["trailing_semicolon"], b"")
    got, types, stats = device_read(engine, good)  # ... and without the bad line: one read, from 1.7 M lines
    assert got[0] == [b"same-read-again-and-again"] and got[1].tolist() == [1000] and got[2].tolist() == [0, 5]
    assert got[3].tolist() == [[0, 12], [995, 1000], [2, 3], [5, 6], [8, 9]] and stats["n_records"] == len(good) // len(row)


def test_compressed_and_missing_files_are_the_callers(engine, tmp_path, golden_dir):
    gz = tmp_path / "truth.yacrd.gz"
    with open(os.path.join(golden_dir, "truth.yacrd"), "rb") as f, gzip.open(gz, "wb") as o:
        o.write(f.read())
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.ingest_report(str(gz), 0.4)
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.ingest_report(str(tmp_path), 0.4)  # a directory: not a regular file


# ---- the CLI -------------------------------------------------------------------------------------------------------------
def cli(args, device=True, ok=True):
    env = dict(os.environ, YACRD_CLI_TIMING="1")
    env.pop("YACRD_NO_DEVICE_REPORT", None)
    if not device:
        env["YACRD_NO_DEVICE_REPORT"] = "1"
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert (p.returncode == 0) == ok, p.stdout + p.stderr
    return p


@pytest.fixture(scope="module")
def work(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("report_cli")
    shutil.copy(os.path.join(golden_dir, "reads.paf"), d / "reads.paf")
    shutil.copy(os.path.join(golden_dir, "truth.yacrd"), d / "truth.yacrd")
    with gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb") as i, open(d / "reads.fastq", "wb") as o:
        shutil.copyfileobj(i, o)
    with open(d / "truth.yacrd", "rb") as i, gzip.open(d / "packed.yacrd.gz", "wb") as o:
        o.write(i.read())
    return d


@pytest.mark.parametrize("sub,src,ext", [("filter", "reads.paf", "paf"), ("scrubb", "reads.fastq", "fastq")])
@pytest.mark.parametrize("report", ["truth.yacrd", "packed.yacrd.gz"])
def test_cli_writes_the_same_bytes_down_either_path(work, sub, src, ext, report):
    outs = {}
    for device in (True, False):
        tag = "%s.%s.%s" % (sub, report.split(".")[0], "dev" if device else "host")
        rep, out = work / (tag + ".yacrd"), work / (tag + "." + ext)
        p = cli(["-i", work / report, "-o", rep, sub, "-i", work / src, "-o", out], device=device)
        info = [l for l in p.stderr.splitlines() if l.startswith("[info] device report reader:")]
        assert len(info) == (1 if device else 0), p.stderr
        if device:
            assert ("(inflated)" in info[0]) == report.endswith(".gz")  # a gzip report takes the _mem route
            assert "230 reads from 230 lines" in info[0]
        outs[device] = (rep.read_bytes(), out.read_bytes())
    assert outs[True] == outs[False]
    assert len(outs[True][0]) > 0 and len(outs[True][1]) > 0


def test_cli_corrupt_report_words_the_host_readers_error_on_both_paths(work):
    bad = work / "bad.yacrd"
    bad.write_bytes(rc.corrupt_text("empty_begin"))
    got = []
    for device in (True, False):
        p = cli(["-i", bad, "-o", work / "bad.out.yacrd"], device=device, ok=False)
        assert "seems corrupt at line 4" in p.stderr and "[info] device report reader" not in p.stderr
        got.append((p.returncode, [l for l in p.stderr.splitlines() if "corrupt" in l]))
    assert got[0] == got[1]
