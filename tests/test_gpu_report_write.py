"""The device report writer (csrc/gpu_report_write.hip: yacrd_engine_write_report / _mem, Engine.write_report / report_text)
against the host writer (yacrd_report_write) on the same arrays: whole byte strings.  What must fall back does, leaves nothing
and leaves the engine usable; the bytes do not depend on the segment size; the CLI writes the same bytes down either path."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import report_cases as rc
import report_write_cases as wc
import yacrd_amd
from yacrd_amd import host
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


def result_of(t):
    return yacrd_amd.Result(t.bad_offsets, t.bad_regions, t.read_type)


def both_forms(e, t, tmp, want=None):
    """the table through write_report and report_text: both equal the host writer's bytes (returned)"""
    if want is None:
        want = wc.host_write(str(tmp / "host.yacrd"), t)
    out = tmp / "dev.yacrd"
    st = e.write_report(str(out), t.names, t.lengths, result_of(t))
    assert out.read_bytes() == want
    assert st["resident"] == 0 and st["n_reads"] == len(t.names) and st["n_regions"] == len(t.bad_regions) and st["text_bytes"] == len(want)
    assert e.report_text(t.names, t.lengths, result_of(t)) == want
    assert not [n for n in os.listdir(tmp) if n.startswith("dev.yacrd.")]  # (no file left beside it)
    return want


def golden(e, golden_dir, tmp):
    """the golden PAF ingested, the resident report against the host writer on the arrays that came home"""
    res, names, lengths, _ = e.ingest_paf(os.path.join(golden_dir, "reads.paf"), 4, 0.4)
    t = wc.Table([n.encode() for n in names], lengths, res.bad_offsets, res.bad_regions, res.read_type)
    want = wc.host_write(str(tmp / "golden.host.yacrd"), t)
    out = tmp / "golden.dev.yacrd"
    st = e.write_report(str(out))
    assert st["resident"] == 1 and st["n_reads"] == len(names) and out.read_bytes() == want and len(want) > 5000
    return t, want


def test_golden_file_resident_and_table_forms(engine, golden_dir, tmp_path):
    t, want = golden(engine, golden_dir, tmp_path)
    assert engine.report_text() == want and engine.report_write_stats["resident"] == 1
    both_forms(engine, t, tmp_path, want)
    assert engine.report_text() == want  # (the table form leaves the resident table alone)


def test_one_engine_through_every_text_path_and_trim(golden_dir, tmp_path):
    """parser, editor (from the mirror), encoder, report reader and report writer on ONE engine, trim, the same again: the
    engine's registry of their buffers is walked with every slot live, by trim and by the engine's end.  The library's count
    of the bytes it holds (live_bytes) says what each trim gave back and that the engine's end gives back everything"""
    paf, rep = os.path.join(golden_dir, "reads.paf"), os.path.join(golden_dir, "truth.yacrd")

    def flat(res, names, lengths):
        return [np.array(res.bad_offsets), np.array(res.bad_regions), np.array(res.read_type), list(names), np.array(lengths)]

    def every_path(e, tag):
        res, names, lengths, _ = e.ingest_paf(paf, 4, 0.4)
        out = tmp_path / (tag + ".paf")
        st = e.edit_overlaps(1, paf, str(out), names, res.read_type)
        assert st["mirror_reused"] == 1
        kept = out.read_bytes()
        blob = e.gzip(kept)
        res2, names2, lengths2, _ = e.ingest_report(rep, 0.4)
        dev = tmp_path / (tag + ".yacrd")
        assert e.write_report(str(dev))["resident"] == 1
        table = e.report_text([n.encode() for n in names], lengths, res)
        return flat(res, names, lengths) + [kept, blob] + flat(res2, names2, lengths2) + [dev.read_bytes(), table]

    live_before = live_bytes()
    with yacrd_amd.Engine(device_id=0) as e:
        first = every_path(e, "first")
        e.trim()
        live_trimmed = live_bytes()
        again = every_path(e, "again")
        e.trim()
        # (the batch path's buffers are grow-only and the inputs were the same: the text paths' scratch is all that came and went)
        assert live_bytes() == live_trimmed
        assert len(first) == len(again) == 14
        for a, b in zip(first, again):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        kept, blob = first[5], first[6]
        assert 0 < len(kept) < os.path.getsize(paf) and len(blob) > 28 and len(first[12]) > 5000 and len(first[13]) > 5000
        # an open gzip writer holds the encoder's buffers: trim leaves them alone, and the writer ends with the right bytes
        gz = tmp_path / "kept.gz"
        w = e.gzip_writer(str(gz))
        w.write(kept[:len(kept) // 2])
        e.trim()
        live_writer_open = live_bytes()
        w.write(kept[len(kept) // 2:])
        w.close()
        assert gz.read_bytes() == blob
        assert not [n for n in os.listdir(tmp_path) if ".gz." in n or ".yacrd." in n or ".paf." in n]
        e.trim()
        assert live_writer_open[0] > live_bytes()[0]  # (the trim under the open writer left the encoder's buffers)
    assert live_bytes() == live_before


def test_fuzz_tables_equal_the_host_writer(engine, tmp_path):
    for seed in range(300):
        t = wc.make_table(seed, tmp_path)
        want = wc.host_write(str(tmp_path / "host.yacrd"), t)
        try:
            got = engine.report_text(t.names, t.lengths, result_of(t))
        except yacrd_amd.NeedsHostParser as x:
            pytest.fail("seed %d fell back: %s" % (seed, x))
        assert got == want, "seed %d differs from the host writer" % seed


def test_round_trip_on_the_device(engine):
    for seed in (3, 17, 59, 119):  # (59, 119: texts on a tile and on the chunk border)
        text = rc.make_text(seed, rc.fuzz_sizes(seed))
        res, names, lengths, _ = engine.ingest_report(text, 0.4)
        first = ([s.encode("utf-8", "surrogateescape") for s in names], lengths, res.bad_offsets, res.bad_regions)
        again = engine.report_text()
        assert engine.report_write_stats["resident"] == 1
        res2, names2, lengths2, _ = engine.ingest_report(again, 0.4)
        second = ([s.encode("utf-8", "surrogateescape") for s in names2], lengths2, res2.bad_offsets, res2.bad_regions)
        assert rc.same(first, second) and np.array_equal(res.read_type, res2.read_type), "seed %d" % seed
        assert again == wc.restate(wc.Table(first[0], lengths, res.bad_offsets, res.bad_regions, res.read_type))


def test_edge_table(engine, tmp_path):
    t = wc.edge_table()
    want = both_forms(engine, t, tmp_path)
    assert want == wc.restate(t)


@pytest.mark.parametrize("r", range(len(wc.edge_table().names)))
def test_edge_table_one_read_per_case(engine, tmp_path, r):
    e = wc.edge_table()
    a, b = int(e.bad_offsets[r]), int(e.bad_offsets[r + 1])
    t = wc.Table([e.names[r]], e.lengths[r:r + 1], np.array([0, b - a], np.uint64), e.bad_regions[a:b], e.read_type[r:r + 1])
    assert engine.report_text(t.names, t.lengths, result_of(t)) == wc.host_write(str(tmp_path / "h.yacrd"), t)


def test_degenerate_tables(engine, tmp_path):
    none = wc.table([], [], [], [])
    out = tmp_path / "empty.yacrd"
    st = engine.write_report(str(out), none.names, none.lengths, result_of(none))
    assert out.exists() and out.read_bytes() == b"" and st["text_bytes"] == 0
    assert engine.report_text(none.names, none.lengths, result_of(none)) == b""
    assert wc.host_write(str(tmp_path / "empty.host.yacrd"), none) == b""
    for one in (wc.table([b"only"], [77], [[]], [2]), wc.table([b"only"], [77], [[(1, 5), (9, 77)]], [1])):
        both_forms(engine, one, tmp_path)


def long_read_table():
    regs = [(3 * k, 3 * k + 2) for k in range(100000)]
    return wc.table([b"before", b"long", b"behind"], [1000, 4000000000, 1000], [[(0, 12), (995, 1000)], regs, [(5, 6)]], [0, 1, 2])


def test_one_read_of_100000_regions_between_two_ordinary_reads(engine, tmp_path):
    want = both_forms(engine, long_read_table(), tmp_path)
    assert len(want) > 1500000 and want.count(b"\n") == 3


def border_table():
    """~1 MB of lines of 20 to 5 000 bytes: ids of 1 to 3 000 bytes, 0 to 150 regions"""
    rng = np.random.RandomState(20241118)
    names, lengths, regs = [], [], []
    total = 0
    while total < 1000000:
        kind = rng.randint(4)
        idl = int(rng.randint(1, 8)) if kind else int(rng.randint(8, 3000))
        n_reg = 0 if kind == 1 else int(rng.randint(0, 6)) if kind else int(rng.randint(0, 150))
        names.append(bytes(rng.choice(np.frombuffer(b"ACGTacgt0123456789_/:.-;,", np.uint8), idl).tolist()))
        lengths.append(int(rng.randint(0, 10 ** int(rng.randint(1, 10)))))
        regs.append([(int(b), int(b) + int(rng.randint(1, 5000))) for b in rng.randint(0, 1 << 20, n_reg)])
        total += 14 + idl + 20 * n_reg
    return wc.table(names, lengths, regs, [i % 3 for i in range(len(names))])


def test_segment_borders_do_not_change_the_bytes(engine, tmp_path, monkeypatch):
    tables = [border_table(), long_read_table()]
    monkeypatch.delenv("YACRD_TEST_REPORT_SEGMENT", raising=False)
    wants = [both_forms(engine, t, tmp_path) for t in tables]
    lines = [len(l) + 1 for l in wants[0].split(b"\n")[:-1]]
    assert 900000 < len(wants[0]) < 1300000 and min(lines) <= 20 and max(lines) >= 5000 > 4096
    monkeypatch.setenv("YACRD_TEST_REPORT_SEGMENT", "4096")  # (read at call time)
    for t, want in zip(tables, wants):
        both_forms(engine, t, tmp_path, want)
    monkeypatch.setenv("YACRD_TEST_REPORT_SEGMENT", "4097")  # ... and borders that fall on no power of two
    both_forms(engine, tables[0], tmp_path, wants[0])


# ---- what falls back leaves nothing and leaves the engine usable ---------------------------------------------------------
def test_fallbacks_leave_nothing_and_the_engine_usable(golden_dir, tmp_path):
    with yacrd_amd.Engine(device_id=0) as e:
        d = tmp_path / "fb"
        d.mkdir()
        with pytest.raises(yacrd_amd.NeedsHostParser):  # a fresh engine: no table is resident
            e.write_report(str(d / "fresh.yacrd"))
        t, want = golden(e, golden_dir, tmp_path)
        bad = t._replace(read_type=np.where(np.arange(len(t.names)) == 100, 3, t.read_type).astype(np.uint8))
        with pytest.raises(yacrd_amd.NeedsHostParser):  # a type of 3
            e.write_report(str(d / "type3.yacrd"), bad.names, bad.lengths, result_of(bad))
        with pytest.raises(yacrd_amd.NeedsHostParser):
            e.report_text(bad.names, bad.lengths, result_of(bad))
        (d / "a_dir").mkdir()
        with pytest.raises(yacrd_amd.NeedsHostParser):  # out_path is a directory
            e.write_report(str(d / "a_dir"), t.names, t.lengths, result_of(t))
        with pytest.raises(yacrd_amd.NeedsHostParser):  # ... or lies in a directory that does not exist
            e.write_report(str(d / "missing" / "r.yacrd"), t.names, t.lengths, result_of(t))
        assert e.report_text() == want  # (none of these disturbed the resident table)
        e.trim()
        with pytest.raises(yacrd_amd.NeedsHostParser):  # after trim()
            e.write_report(str(d / "trimmed.yacrd"))
        golden(e, golden_dir, tmp_path)
        off, iv, lens = host.synth_csr(host.SYNTH_ONT, 300, 6000, 20241110)
        e.run(off, iv, lens, 4, 0.4)
        with pytest.raises(yacrd_amd.NeedsHostParser):  # after a run that followed the ingest
            e.report_text()
        with pytest.raises(yacrd_amd.NeedsHostParser):
            e.write_report(str(d / "after_run.yacrd"))
        assert sorted(os.listdir(d)) == ["a_dir"] and os.listdir(d / "a_dir") == []
        golden(e, golden_dir, tmp_path)  # the engine is as usable as before
        both_forms(e, t, tmp_path, want)


def test_a_failed_run_or_stream_finish_leaves_no_table_resident(golden_dir, tmp_path):
    """A call that fails after it has rewritten (or moved) the engine's lengths must not leave the earlier ingest's table
    looking resident: the resident form falls back, nothing is written, and the next ingest serves again."""
    with yacrd_amd.Engine(device_id=0) as e:
        d = tmp_path / "stale"
        d.mkdir()
        t, want = golden(e, golden_dir, tmp_path)
        R = len(t.names)
        bad = np.zeros(4, dtype=yacrd_amd.OVL_REC_DTYPE)
        bad["ea"], bad["eb"] = 5, 5
        for n_reads in (R, 100000):  # as many reads as the table (the lengths are overwritten in place), many more (they move)
            bad["b"][2] = n_reads + 5  # a read outside the table: found after the lengths went up
            with yacrd_amd.Stream(e, 999, 2) as st:
                st.push(bad)
                with pytest.raises(yacrd_amd.EngineError, match="outside"):
                    st.finish(None, np.full(n_reads, 7, np.uint32), 2, 0.4)
            with pytest.raises(yacrd_amd.NeedsHostParser):
                e.report_text()
            with pytest.raises(yacrd_amd.NeedsHostParser):
                e.write_report(str(d / "after_finish.yacrd"))
            golden(e, golden_dir, tmp_path)
        with pytest.raises(yacrd_amd.EngineError, match=r"offsets\[0\]"):  # a run refused at its door
            e.run(np.array([1, 1], np.uint64), np.zeros((1, 2), np.uint32), np.array([9], np.uint32), 4, 0.4)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            e.write_report(str(d / "after_run.yacrd"))
        assert os.listdir(d) == []
        golden(e, golden_dir, tmp_path)
        assert e.report_text() == want


def test_an_existing_output_keeps_its_mode_and_in_place_cases_fall_back(golden_dir, tmp_path):
    """The device writer renames over out_path where the host writer truncates in place: an existing file keeps its mode,
    and where the difference would show (other hard links, a file that may not be written) the host writer is asked."""
    with yacrd_amd.Engine(device_id=0) as e:
        t, want = golden(e, golden_dir, tmp_path)
        out = tmp_path / "kept.yacrd"
        out.write_bytes(b"old")
        os.chmod(out, 0o640)
        e.write_report(str(out))
        assert out.read_bytes() == want and (os.stat(out).st_mode & 0o7777) == 0o640
        os.link(out, tmp_path / "second_name")
        out.write_bytes(b"old")
        with pytest.raises(yacrd_amd.NeedsHostParser):
            e.write_report(str(out))
        os.unlink(tmp_path / "second_name")
        os.chmod(out, 0o440)
        if not os.access(out, os.W_OK):  # (root may write anything: nothing differs then)
            with pytest.raises(yacrd_amd.NeedsHostParser):
                e.write_report(str(out))
        assert out.read_bytes() == b"old" and not [n for n in os.listdir(tmp_path) if n.startswith("kept.yacrd.")]


# ---- the CLI -------------------------------------------------------------------------------------------------------------
def cli(args, device, extra=None):
    env = dict(os.environ, YACRD_CLI_TIMING="1")
    for k in ("YACRD_NO_DEVICE_REPORT_WRITER", "YACRD_TEST_REPORT_SEGMENT"):
        env.pop(k, None)
    if not device:
        env["YACRD_NO_DEVICE_REPORT_WRITER"] = "1"
    env.update(extra or {})
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


@pytest.mark.parametrize("src,gpus,path", [("reads.paf", 1, "resident table"), ("truth.yacrd", 1, "resident table"),
                                           ("reads.paf", 2, "table uploaded")])
def test_cli_writes_the_same_report_down_either_path(golden_dir, tmp_path, src, gpus, path):
    shutil.copy(os.path.join(golden_dir, src), tmp_path / src)
    outs = []
    for device in (True, False):
        out = tmp_path / ("dev.yacrd" if device else "host.yacrd")
        p = cli(["-i", tmp_path / src, "-o", out, "-c", 4, "-n", 0.4, "--gpus", gpus], device, {"YACRD_GPUS_ON_DEVICE": "0"})
        info = [l for l in p.stderr.splitlines() if l.startswith("[info] device report writer:")]
        assert len(info) == (1 if device else 0), p.stderr
        assert ("[info] host report writer" in p.stderr) == (not device)
        if device:
            assert path in info[0] and "230 reads" in info[0], info[0]
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] and outs[0].count(b"\n") == 230


def test_cli_filter_behind_the_device_writer_still_edits_from_the_mirror(golden_dir, tmp_path):
    shutil.copy(os.path.join(golden_dir, "reads.paf"), tmp_path / "reads.paf")
    outs = []
    for device in (True, False):
        tag = "dev" if device else "host"
        p = cli(["-i", tmp_path / "reads.paf", "-o", tmp_path / (tag + ".yacrd"), "-c", 4, "-n", 0.4, "filter", "-i", tmp_path / "reads.paf",
                 "-o", tmp_path / (tag + ".paf")], device)
        assert "mirror_reused=1" in p.stderr, p.stderr  # (the writer ran in between and left the parser's mirror valid)
        outs.append(((tmp_path / (tag + ".yacrd")).read_bytes(), (tmp_path / (tag + ".paf")).read_bytes()))
    assert outs[0] == outs[1]
