"""filter / extract on overlap files on the GPU (yacrd_engine_edit_overlaps, csrc/gpu_edit.hip).  The yardstick for bytes is
the host loop (yacrd_edit_file: host.edit_file, or the CLI under YACRD_NO_DEVICE_EDITOR=1) and the ten-line restatement
that tests/test_edit_overlaps.py pins to it on the CPU — never the device path itself."""
import gzip
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import yacrd_amd
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, fuzz_cases, host_loop, restate
from yacrd_amd import host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")

# the reference's unit vectors (src/editor/filter.rs:289-359, extract.rs:293-362) and their three reads, read 1 bad
_PAF_UNIT = ("1\t12000\t20\t4500\t-\t2\t10000\t5500\t10000\t4500\t4500\t255\n"
             "1\t12000\t5500\t10000\t-\t3\t10000\t0\t4500\t4500\t4500\t255\n")
_M4_UNIT = "1 2 0.1 2 0 100 450 1000 0 550 900 1000\n1 3 0.1 2 0 550 900 1000 0 100 450 1000\n"
_UNIT_NAMES, _UNIT_TYPES = [b"1", b"2", b"3"], [yacrd_amd.NOT_COVERED, yacrd_amd.NOT_BAD, yacrd_amd.NOT_BAD]


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


@pytest.mark.parametrize("op", [OP_FILTER, OP_EXTRACT])
@pytest.mark.parametrize("ext,text", [(".paf", _PAF_UNIT), (".m4", _M4_UNIT), (".mhap", _M4_UNIT)])
def test_reference_unit_vectors(engine, op, ext, text):
    fmt = 1 if ext == ".paf" else 2
    text = text.encode()
    # every line names read 1: filter drops them all, extract keeps them all
    assert engine.edit_overlaps_text(op, text, _UNIT_NAMES, _UNIT_TYPES, fmt) == (b"" if op == OP_FILTER else text)
    assert engine.edit_stats["n_lines"] == 2 and engine.edit_stats["n_kept"] == (0 if op == OP_FILTER else 2)
    more = text + (b"2\t1000\t0\t500\t+\t3\t1000\t500\t1000\t500\t500\t255\n" if fmt == 1 else b"2 3 0.1 2 0 0 500 1000 0 500 1000 1000\n")
    assert engine.edit_overlaps_text(op, more, _UNIT_NAMES, _UNIT_TYPES, fmt) == (more[len(text):] if op == OP_FILTER else text)


def test_reference_unit_vectors_by_file_name(engine, tmp_path):
    for ext, text in ((".paf", _PAF_UNIT), (".m4", _M4_UNIT), (".mhap", _M4_UNIT)):
        src, out = tmp_path / ("u" + ext), tmp_path / ("o" + ext)
        src.write_text(text)
        st = engine.edit_overlaps(OP_EXTRACT, str(src), str(out), _UNIT_NAMES, _UNIT_TYPES)
        assert out.read_text() == text and st["n_kept"] == 2 and st["kept_bytes"] == len(text)


_PIECE = 4 << 20  # what one trip home of the kept bytes carries (csrc/gpu_edit.hip: kOutPiece)


def _lines_of_64(fmt, total):
    """`total` bytes of identical 64-byte lines, the last one's final column a character longer or shorter where needed"""
    head = b"a\t12000\t20\t4500\t-\tb\t10000\t5500\t10000\t4500\t4500\t" if fmt == 1 else b"a b 0.1 2 0 100 450 1000 0 550 900 "
    line = head + b"7" * (63 - len(head)) + b"\n"
    n_lines = (total + 32) // 64
    last = head + b"7" * (63 - len(head) + total - 64 * n_lines) + b"\n"
    text = line * (n_lines - 1) + last
    assert len(line) == 64 and len(text) == total and abs(len(last) - 64) <= 1
    return text, n_lines


@pytest.mark.parametrize("fmt", [1, 2], ids=["paf", "m4"])
@pytest.mark.parametrize("total", [_PIECE - 1, _PIECE, _PIECE + 1, 2 * _PIECE + 1])
def test_piece_borders_of_the_way_home(engine, tmp_path, fmt, total):
    """everything is kept (filter, no read is bad): the kept bytes end one byte before, on and one byte behind a piece
    border of the way home, and behind two pieces — out of memory, into a file and through the encoder"""
    text, n_lines = _lines_of_64(fmt, total)
    assert engine.edit_overlaps_text(OP_FILTER, text, [], [], fmt) == text
    assert engine.edit_stats["n_kept"] == n_lines and engine.edit_stats["kept_bytes"] == total
    src, out = tmp_path / ("in" + (".paf" if fmt == 1 else ".m4")), tmp_path / "out.txt"
    src.write_bytes(text)
    st = engine.edit_overlaps(OP_FILTER, str(src), str(out), [], [])
    assert out.read_bytes() == text and st["kept_bytes"] == total and st["n_kept"] == n_lines
    assert gzip.decompress(engine.edit_overlaps_gzip(OP_FILTER, text, [], [], fmt)) == text
    assert engine.gzip_stats["in_bytes"] == total
    assert sorted(os.listdir(tmp_path)) == sorted([src.name, out.name])


def _streams_equal(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 22), fb.read(1 << 22)
            if x != y:
                return False
            if not x:
                return True


@pytest.mark.parametrize("cov,ncov,n_bad_lines", [(0, 0.8, 57), (4, 0.4, 448)])
def test_fixture_against_the_host_loop(engine, golden_dir, tmp_path, cov, ncov, n_bad_lines):
    paf = os.path.join(golden_dir, "reads.paf")
    res, names, lengths, _ = engine.ingest_paf(paf, cov, ncov)
    for op in (OP_FILTER, OP_EXTRACT):
        want, got = str(tmp_path / "host.paf"), str(tmp_path / "dev.paf")
        host.edit_file(op, paf, want, names, lengths, res.bad_offsets, res.bad_regions, res.read_type, n_threads=1)
        st = engine.edit_overlaps(op, paf, got, names, res.read_type)
        assert _streams_equal(want, got), op
        assert st["n_lines"] == 1286 and 0 < st["n_kept"] < st["n_lines"]
        assert st["n_kept"] == (1286 - n_bad_lines if op == OP_FILTER else n_bad_lines)
        assert st["kept_bytes"] == os.path.getsize(want) and st["text_bytes"] == os.path.getsize(paf)


def test_fuzz_zero_fallbacks(engine, tmp_path):
    """every text of the fuzz set is taken by the device path (no NeedsHostParser: a path that falls back on plain text
    hides behind the host loop), bytes are the host loop's, counts are the restatement's"""
    n = 0
    for tag, text, m4, names, types in fuzz_cases():
        table = dict(zip(names, types))
        for op in (OP_FILTER, OP_EXTRACT):
            got = engine.edit_overlaps_text(op, text, names, types, 2 if m4 else 1)  # (raises on YACRD_EFALLBACK)
            want, n_lines, n_kept = restate(text, op, table, m4)
            assert got == want, (tag, m4, op, len(text))
            assert got == host_loop(str(tmp_path), op, text, names, types, ".m4" if m4 else ".paf"), (tag, m4, op)
            st = engine.edit_stats
            assert (st["kept_bytes"], st["n_kept"], st["n_lines"], st["text_bytes"]) == (len(want), n_kept, n_lines, len(text)), (tag, m4, op)
        n += 1
    assert n >= 1000


def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


_GOOD = b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\t255\n"
_FALLBACKS = [
    ("quote", ".paf", _GOOD + b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\t\"x\"\n"),
    ("crlf", ".paf", _GOOD.replace(b"\n", b"\r\n") * 3),
    ("lone_cr", ".paf", _GOOD + b"a\t10\t0\t5\t+\tb\t10\t0\r5\t5\t5\t255\n"),
    ("field_count", ".paf", _GOOD * 3 + b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\n" + _GOOD),
    ("too_few_fields", ".paf", b"a\t10\t0\t5\t+\n" * 2),
    ("too_few_fields_m4", ".m4", b"a\n"),
    ("gz", ".paf.gz", gzip.compress(_GOOD * 4)),
]


@pytest.mark.parametrize("op", ["filter", "extract"])
@pytest.mark.parametrize("tag,ext,text", _FALLBACKS, ids=[f[0] for f in _FALLBACKS])
def test_what_must_fall_back_does_and_writes_nothing(engine, tmp_path, op, tag, ext, text):
    d = tmp_path / "dev"
    d.mkdir()
    src, out = tmp_path / ("in" + ext), d / ("out" + ext)
    src.write_bytes(text)
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.edit_overlaps(OP_FILTER if op == "filter" else OP_EXTRACT, str(src), str(out), [b"a"], [1])
    assert os.listdir(d) == []
    if ext != ".paf.gz":
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps_text(OP_FILTER if op == "filter" else OP_EXTRACT, text, [b"a"], [1], 2 if ext == ".m4" else 1)
    # the CLI still does what the parent does: the host loop's bytes, or its error and exit status
    rep = tmp_path / "in.yacrd"
    rep.write_text("Chimeric\ta\t10\t2,4,6\nNotBad\tb\t10\t\n")
    runs = []
    for env in ({"YACRD_NO_DEVICE_EDITOR": "1"}, {}):
        o = tmp_path / ("cli%d" % len(runs) + ext)
        p = _cli(["-i", rep, "-o", tmp_path / "again.yacrd", op, "-i", src, "-o", o], YACRD_CLI_TIMING="1", **env)
        runs.append((p.returncode, [l for l in p.stderr.splitlines() if l.startswith("Error")],
                     o.read_bytes() if o.exists() else None))
        assert "[info] device editor" not in p.stderr
    assert runs[0] == runs[1]


def test_long_ids_and_many_reads(engine):
    """a table of 200 000 reads (the open-addressing table well filled), every id looked up"""
    names = [b"read_%07d/%d" % (i, i * 7919 % 1000) for i in range(200_000)]
    types = np.array([(i * 2654435761 >> 7) % 3 for i in range(len(names))], np.uint8)
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, len(names) + 50_000, 60_000), rng.integers(0, len(names) + 50_000, 60_000)
    nm = lambda i: names[i] if i < len(names) else b"absent_%d" % i
    text = b"".join(b"%s\t9\t0\t5\t+\t%s\t9\t0\t5\t5\t5\t255\n" % (nm(int(x)), nm(int(y))) for x, y in zip(a, b))
    table = dict(zip(names, types.tolist()))
    for op in (OP_FILTER, OP_EXTRACT):
        want, n_lines, n_kept = restate(text, op, table, False)
        assert engine.edit_overlaps_text(op, text, names, types, 1) == want
        assert 0 < n_kept < n_lines and engine.edit_stats["n_kept"] == n_kept


@pytest.fixture(scope="module")
def synth():
    d = "/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp"
    tag = os.path.join(d, "yacrd_edit_test_%d_" % os.getpid())
    paf = tag + "s.paf"
    host.synth_paf(host.SYNTH_SEQUEL, 50_000, 5_000_000, 20241108 + 5, paf)
    made = [paf]
    yield paf, tag, made
    for x in made:
        if os.path.exists(x):
            os.remove(x)


def test_synthetic_file_at_size(synth):
    paf, tag, made = synth
    with yacrd_amd.Engine(device_id=0) as e:
        res, names, lengths, _ = e.ingest_paf(paf, 3, 0.4)
        types = res.read_type
        assert (types == 1).sum() > 500 and (types == 2).sum() > 500
        for op in (OP_FILTER, OP_EXTRACT):
            want, got = tag + "host%d.paf" % op, tag + "dev%d.paf" % op
            made.extend([want, got])
            t0 = time.perf_counter()
            host.edit_file(op, paf, want, names, lengths, res.bad_offsets, res.bad_regions, types, n_threads=1)
            host_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            st = e.edit_overlaps(op, paf, got, names, types)
            device_s = time.perf_counter() - t0
            print("op %d: host loop %.3f s, device %.3f s (first call), stats %s" % (op, host_s, device_s, st))
            assert _streams_equal(want, got), op
            assert 0 < st["n_kept"] < st["n_lines"] == 5_000_000 and st["kept_bytes"] == os.path.getsize(want)
            assert st["mirror_reused"] == 1  # (the file the engine just parsed)
            assert device_s < host_s
            # once more on the same engine (warm buffers), from a copy of the file: the text is moved
            cp = tag + "copy.paf"
            if cp not in made:
                shutil.copy(paf, cp)
                made.append(cp)
            os.remove(got)
            t0 = time.perf_counter()
            st2 = e.edit_overlaps(op, cp, got, names, types)
            moved_s = time.perf_counter() - t0
            print("op %d: device %.3f s with the text moved, stats %s" % (op, moved_s, st2))
            assert st2["mirror_reused"] == 0 and _streams_equal(want, got), op
            os.remove(got)
            st3 = e.edit_overlaps(op, cp, got, names, types)
            assert _streams_equal(want, got) and st3["kept_bytes"] == st["kept_bytes"]
            assert moved_s < host_s
        e.trim()
        st4 = e.edit_overlaps(OP_FILTER, paf, got, names, types)  # (after trim: no mirror, fresh buffers)
        assert st4["mirror_reused"] == 0 and _streams_equal(tag + "host%d.paf" % OP_FILTER, got)
        e.trim()


def _editor_line(p):
    hit = [l for l in p.stderr.splitlines() if l.startswith("[info] device editor")]
    assert len(hit) == 1, p.stderr
    return hit[0]


@pytest.mark.parametrize("op", ["filter", "extract"])
def test_cli_on_the_fixture(golden_dir, tmp_path, op):
    paf = tmp_path / "reads.paf"
    shutil.copy(os.path.join(golden_dir, "reads.paf"), paf)
    a, b = tmp_path / "dev.paf", tmp_path / "host.paf"
    p = _cli(["-i", paf, "-o", tmp_path / "r.yacrd", "-c", "4", "-n", "0.4", op, "-i", paf, "-o", a], YACRD_CLI_TIMING="1")
    assert p.returncode == 0, p.stderr
    assert "mirror_reused=1" in _editor_line(p)
    q = _cli(["-i", paf, "-o", tmp_path / "r2.yacrd", "-c", "4", "-n", "0.4", op, "-i", paf, "-o", b], YACRD_CLI_TIMING="1",
             YACRD_NO_DEVICE_EDITOR="1")
    assert q.returncode == 0 and "[info] device editor" not in q.stderr
    assert a.read_bytes() == b.read_bytes() and 0 < a.stat().st_size < paf.stat().st_size
    # a copy of the file is another file: the text is moved again; --gpus 2 (on one device) edits on the first engine
    cp = tmp_path / "copy.paf"
    shutil.copy(paf, cp)
    p = _cli(["-i", paf, "-o", tmp_path / "r3.yacrd", "-c", "4", "-n", "0.4", "--gpus", "2", op, "-i", cp, "-o", a],
             YACRD_CLI_TIMING="1", YACRD_GPUS_ON_DEVICE="0")
    assert p.returncode == 0, p.stderr
    assert "mirror_reused=0" in _editor_line(p) and a.read_bytes() == b.read_bytes()


def test_cli_on_the_synthetic_file(synth):
    paf, tag, made = synth
    a, b, rep = tag + "cli_dev.paf", tag + "cli_host.paf", tag + "cli.yacrd"
    made.extend([a, b, rep])
    p = _cli(["-i", paf, "-o", rep, "-c", "4", "-n", "0.4", "filter", "-i", paf, "-o", a], YACRD_CLI_TIMING="1")
    assert p.returncode == 0, p.stderr
    assert "mirror_reused=1" in _editor_line(p)
    q = _cli(["-i", paf, "-o", rep, "-c", "4", "-n", "0.4", "filter", "-i", paf, "-o", b], YACRD_NO_DEVICE_EDITOR="1")
    assert q.returncode == 0, q.stderr
    assert _streams_equal(a, b) and 0 < os.path.getsize(a) < os.path.getsize(paf)
