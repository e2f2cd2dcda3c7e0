"""scrubb / split / filter / extract on FASTQ on the GPU (yacrd_engine_edit_fastq, csrc/gpu_seq_edit.hip).  The yardsticks for
bytes are the host loop (yacrd_edit_file: host.edit_file, or the CLI under YACRD_NO_DEVICE_EDITOR=1), the restatement that
tests/test_edit_fastq_cases.py pins to it and to oracle/editors.py on the CPU, and the reference's truth.*.fastq.gz — never
the device path itself."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import yacrd_amd
from edit_fastq_cases import (CHIMERIC, NOT_COVERED, OPS, OP_EXTRACT, OP_FILTER, OP_NAMES, OP_SCRUBB, OP_SPLIT, OUT_TILE, SEGMENT, TILE, Table,
                              fallback_cases, fuzz_cases, host_loop, restate)
from yacrd_amd import host
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
_PIECE = 4 << 20   # what one trip home of the output carries (csrc/gpu_seq_edit.hip: kOutPiece)
_BLOCK = 65280     # bytes of text per BGZF member (csrc/bgzf_sizes.h: kBlock)
_EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


def _edit(engine, op, text, table):
    names, lengths, bo, br, rt = table.arrays()
    return engine.edit_fastq_text(op, text, names, lengths, (bo, br, rt))


def _edit_file(engine, op, src, out, table):
    names, lengths, bo, br, rt = table.arrays()
    return engine.edit_fastq(op, str(src), str(out), names, lengths, (bo, br, rt))


# ---- the reference's fixture ------------------------------------------------------------------------------------------------
def test_golden_fixture_all_four_ops(engine, golden_dir, tmp_path):
    """The reference's fixture: reads.fastq.gz inflated, the table from ingest_report on truth.yacrd, the reference's
    truth.{scrubb,filter,extract,split}.fastq.gz as the yardstick.  Those four files were written at the reference's default
    -n 0.8 (tests/run.rs; tests/test_oracle_editors.py pins them at 0.8): a table classified at -n 0.4 turns 12 more reads
    NotCovered and does NOT give them — measured on the CPU with the restatement and the host loop alike.  So the truth files
    are compared at 0.8, and the table at -n 0.4 is compared with the host loop, which is its yardstick."""
    text = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read()
    src = tmp_path / "reads.fastq"
    src.write_bytes(text)
    made = ["reads.fastq"]
    for ncov in (0.8, 0.4):
        res, names, lengths, _ = engine.ingest_report(os.path.join(golden_dir, "truth.yacrd"), ncov)
        for op in OPS:
            truth = gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % OP_NAMES[op]), "rb").read()
            if ncov == 0.4:
                want = tmp_path / "host.fastq"
                host.edit_file(op, str(src), str(want), names, lengths, res.bad_offsets, res.bad_regions, res.read_type, n_threads=1)
                truth, was = want.read_bytes(), truth
                want.unlink()
                assert truth != was
            assert engine.edit_fastq_text(op, text, names, lengths, res) == truth, (OP_NAMES[op], ncov)
            st = engine.seq_edit_stats
            assert (st["text_bytes"], st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(text), len(truth), 461, truth.count(b"\n") // 4)
            out = tmp_path / ("out.%s.%s.fastq" % (OP_NAMES[op], ncov))
            made.append(out.name)
            st = engine.edit_fastq(op, str(src), str(out), names, lengths, res)
            assert out.read_bytes() == truth and st["out_bytes"] == len(truth), (OP_NAMES[op], ncov)
    assert sorted(os.listdir(tmp_path)) == sorted(made)


# ---- the fuzz set ---------------------------------------------------------------------------------------------------------------
def test_fuzz_zero_fallbacks(engine, tmp_path):
    """every text of the fuzz set is taken by the device path (no NeedsHostParser: a path that falls back on plain text hides
    behind the host loop), bytes are the host loop's, counts are the restatement's"""
    n = 0
    for tag, text, table in fuzz_cases():
        for op in OPS:
            got = _edit(engine, op, text, table)  # (raises on YACRD_EFALLBACK)
            want, n_in, n_out = restate(text, op, table)
            assert got == want, (tag, op, len(text))
            if len(text) < 100000 or op == OP_SCRUBB:
                assert got == host_loop(str(tmp_path), op, text, table), (tag, op)
            st = engine.seq_edit_stats
            assert (st["text_bytes"], st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(text), len(want), n_in, n_out), (tag, op)
        n += 1
    assert n >= 250


# ---- smallest shapes, text tile borders --------------------------------------------------------------------------------------
def _filler(size):
    """records `@f`, absent from every table, of exactly `size` bytes (>= 14): one record is 2 m + 7 bytes"""
    if size % 2 == 0:
        return b"@f\n\n+\n\n" + _filler(size - 7)
    m = (size - 7) // 2
    assert m >= 0
    return b"@f\n" + b"A" * m + b"\n+\n" + b"#" * m + b"\n"


_TARGET = b"@target of the cut\n" + b"ACGT" * 10 + b"\n+\n" + bytes(range(40, 80)) + b"\n"
_TARGET_TABLE = Table([b"target"], [40], [[(5, 10), (20, 21)]], [CHIMERIC])


def test_empty_text_and_single_records(engine):
    assert _edit(engine, OP_SCRUBB, b"", Table()) == b"" and engine.seq_edit_stats["n_records"] == 0
    one = b"@r d\nACGT\n+\n!!!!\n"
    for op in OPS:
        assert _edit(engine, op, one, Table()) == (b"" if op == OP_EXTRACT else one)
    whole = Table([b"r"], [4], [[(0, 4)]], [CHIMERIC])
    assert _edit(engine, OP_SCRUBB, one, whole) == b""
    assert _edit(engine, OP_SPLIT, one, whole) == b"@r_0_4 d\nACGT\n+\n!!!!\n"
    assert _edit(engine, OP_EXTRACT, one, whole) == one and _edit(engine, OP_FILTER, one, whole) == b""
    assert _edit(engine, OP_SCRUBB, one, Table([b"r"], [4], [[(0, 4)]], [NOT_COVERED])) == b""


@pytest.mark.parametrize("tiles", [1, 2, 3])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_text_of_whole_tiles_and_a_byte(engine, tmp_path, tiles, d):
    """the text's last newline lies before, on and behind a tile border"""
    text = _filler(tiles * TILE + d - len(_TARGET)) + _TARGET
    assert len(text) == tiles * TILE + d
    for op in (OP_SCRUBB, OP_FILTER):
        assert _edit(engine, op, text, _TARGET_TABLE) == host_loop(str(tmp_path), op, text, _TARGET_TABLE)


@pytest.mark.parametrize("what,before", [("header", 3), ("header_newline", len(b"@target of the cut")), ("sequence", 30), ("plus", 19 + 41),
                                          ("plus_newline", 19 + 42), ("quality", 19 + 41 + 2 + 7), ("last_newline", len(_TARGET) - 1)])
def test_a_line_straddles_a_tile_border(engine, tmp_path, what, before):
    """byte `before` of the cut record is the first of the second tile"""
    text = _filler(TILE - before) + _TARGET + _filler(100)
    assert text[TILE - before:].startswith(_TARGET)
    for op in OPS:
        assert _edit(engine, op, text, _TARGET_TABLE) == host_loop(str(tmp_path), op, text, _TARGET_TABLE), (what, op)


def test_a_record_of_100000_bases(engine, tmp_path):
    rng = np.random.default_rng(3)
    n = 100000
    rec = b"@long one\n" + bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]) + b"\n+\n" + bytes(rng.integers(33, 127, n, dtype=np.uint8)) + b"\n"
    text = _filler(1001) + rec + _filler(77)
    table = Table([b"long"], [n], [[(0, 7), (32768, 65536), (65536, 65537), (99999, 100000)]], [CHIMERIC])
    for op in OPS:
        assert _edit(engine, op, text, table) == host_loop(str(tmp_path), op, text, table), op


# ---- output borders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_output_of_whole_tiles_and_a_byte(engine, k, d):
    """everything is copied: the output ends one byte before, on and one byte behind an output tile border"""
    text = _filler(k * OUT_TILE + d)
    assert _edit(engine, OP_SCRUBB, text, _TARGET_TABLE) == text and engine.seq_edit_stats["out_bytes"] == k * OUT_TILE + d


@pytest.mark.parametrize("before", [1, 3, 8, 12, 14, 19, 25])
def test_a_cut_header_straddles_an_output_tile_border(engine, tmp_path, before):
    """the copied records in front fill the first output tile but `before` bytes: `@target_0_5 of the cut` lies across the border"""
    text = _filler(OUT_TILE - before) + _TARGET
    for op in (OP_SCRUBB, OP_SPLIT):
        got = _edit(engine, op, text, _TARGET_TABLE)
        assert got == host_loop(str(tmp_path), op, text, _TARGET_TABLE), op
        assert got[OUT_TILE - before:].startswith(b"@target_0_5 of the cut\nACGTA\n+\n")


def _records_of_1k(total):
    rec = b"@r%04d\n" % 7 + b"ACGT" * 126 + b"\n+\n" + b"I" * 504 + b"\n"
    assert len(rec) == 1019
    n = total // len(rec) - 1
    return rec * n + _filler(total - n * len(rec)), n


@pytest.mark.parametrize("total", [_PIECE - 1, _PIECE, _PIECE + 1, 2 * _PIECE + 1])
def test_piece_borders_of_the_way_home(engine, tmp_path, total):
    """everything is kept: the output ends one byte before, on and one byte behind a piece border of the way home, and behind
    two pieces — out of memory, into a file and through the encoder"""
    text, _ = _records_of_1k(total)
    assert len(text) == total
    assert _edit(engine, OP_FILTER, text, Table()) == text and engine.seq_edit_stats["out_bytes"] == total
    src, out = tmp_path / "in.fastq", tmp_path / "out.fastq"
    src.write_bytes(text)
    st = _edit_file(engine, OP_SCRUBB, src, out, Table())
    assert out.read_bytes() == text and st["out_bytes"] == total and st["n_records"] == st["n_out_records"] == text.count(b"\n") // 4
    assert gzip.decompress(engine.edit_fastq_gzip(OP_FILTER, text, [], [], ([0], [], []))) == text
    assert engine.gzip_stats["in_bytes"] == total
    assert sorted(os.listdir(tmp_path)) == ["in.fastq", "out.fastq"]


# ---- the segment border ---------------------------------------------------------------------------------------------------------
def _streams_equal(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 22), fb.read(1 << 22)
            if x != y:
                return False
            if not x:
                return True


@pytest.fixture(scope="module")
def big_prefix():
    """good records, `ok` cut under scrubb, up to 200 bytes short of the mover's first segment border"""
    block = (b"@ok a b\nACGTACGTAC\n+\n!!!!!!!!!!\n" + _filler(993)) * 1024
    reps = (SEGMENT - 200) // len(block)
    body = block * reps
    return body + _filler(SEGMENT - 200 - len(body))


def test_records_across_the_segment_border(engine, big_prefix):
    """a text just over 128 MiB + 4 MiB: a cut record whose sequence straddles the segment border — its pieces come from both
    sides — with a copied record's bytes on both sides too; against the host loop, compared in streams"""
    d = "/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp"
    tag = os.path.join(d, "yacrd_seq_edit_test_%d_" % os.getpid())
    n = 1000
    wide = b"@wide w\n" + b"ACGT" * (n // 4) + b"\n+\n" + bytes(33 + i % 90 for i in range(n)) + b"\n"
    tail = (b"@ok a b\nACGTACGTAC\n+\n!!!!!!!!!!\n" + _filler(993)) * (4 * 1024 + 7)
    text = big_prefix + wide + tail
    assert len(big_prefix) == SEGMENT - 200 and SEGMENT + (4 << 20) < len(text) < SEGMENT + (5 << 20)
    table = Table([b"ok", b"wide"], [10, n], [[(2, 4)], [(100, 150), (400, 600)]], [CHIMERIC, CHIMERIC])
    names, lengths, bo, br, rt = table.arrays()
    src, want, got = tag + "in.fastq", tag + "host.fastq", tag + "dev.fastq"
    try:
        with open(src, "wb") as f:
            f.write(text)
        for op in (OP_SCRUBB, OP_FILTER):
            host.edit_file(op, src, want, names, lengths, bo, br, rt)
            st = engine.edit_fastq(op, src, got, names, lengths, (bo, br, rt))
            assert _streams_equal(want, got), op
            assert st["out_bytes"] == os.path.getsize(want) and st["text_bytes"] == len(text)
            if op == OP_FILTER:  # (both reads are Chimeric: only the fillers stay)
                assert st["n_out_records"] < st["n_records"]
            os.remove(got)
    finally:
        for x in (src, want, got):
            if os.path.exists(x):
                os.remove(x)
        engine.trim()


def test_a_table_of_200000_reads(engine, tmp_path):
    names = [b"read_%07d/%d" % (i, i * 7919 % 1000) for i in range(200_000)]
    types = [(i * 2654435761 >> 7) % 3 for i in range(len(names))]
    regions = [[(3, 9)] if i % 3 else [] for i in range(len(names))]
    table = Table(names, [12] * len(names), regions, types)
    rng = np.random.default_rng(5)
    pick = rng.integers(0, len(names) + 50_000, 40_000)
    text = b"".join(b"@%s\nACGTACGTACGT\n+\n0123456789ab\n" % (names[i] if i < len(names) else b"absent_%d" % i) for i in pick.tolist())
    for op in OPS:
        want, n_in, n_out = restate(text, op, table)
        assert _edit(engine, op, text, table) == want
        assert 0 < n_out and engine.seq_edit_stats["n_out_records"] == n_out and n_in == 40_000
    assert _edit(engine, OP_SCRUBB, text, table) == host_loop(str(tmp_path), OP_SCRUBB, text, table)


# ---- what falls back ----------------------------------------------------------------------------------------------------------------
_FALLBACKS = fallback_cases()


@pytest.mark.parametrize("tag,ops,text,table", _FALLBACKS, ids=[f[0] for f in _FALLBACKS])
def test_what_must_fall_back_does_and_writes_nothing(engine, tmp_path, tag, ops, text, table):
    d = tmp_path / "dev"
    d.mkdir()
    src, out = tmp_path / "in.fastq", d / "out.fastq"
    src.write_bytes(text)
    for op in ops:
        with pytest.raises(yacrd_amd.NeedsHostParser):
            _edit(engine, op, text, table)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            _edit_file(engine, op, src, out, table)
        assert os.listdir(d) == []
    out.write_bytes(b"what was there")
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _edit_file(engine, ops[0], src, out, table)
    assert os.listdir(d) == ["out.fastq"] and out.read_bytes() == b"what was there"
    with pytest.raises(yacrd_amd.NeedsHostParser):
        names, lengths, bo, br, rt = table.arrays()
        engine.edit_fastq_gzip(ops[0], text, names, lengths, (bo, br, rt), out_path=str(d / "out.fastq.gz"))
    assert os.listdir(d) == ["out.fastq"]


def test_fallback_causes_behind_the_first_segment(engine, big_prefix):
    """the same causes behind the first 128 MiB of good records"""
    try:
        assert len(_edit(engine, OP_FILTER, big_prefix, _FALLBACKS[0][3])) > 0  # (the prefix alone is taken)
        for tag, ops, text, table in _FALLBACKS:
            with pytest.raises(yacrd_amd.NeedsHostParser):
                _edit(engine, ops[0], big_prefix + b"@f\nACGT\n+\n!!!!\n" * 50 + text, table)
    finally:
        engine.trim()


def test_other_inputs_of_the_file_form_fall_back(engine, tmp_path):
    good = b"@r\nACGT\n+\n!!!!\n"
    d = tmp_path / "dev"
    d.mkdir()
    for name, blob in (("in.fastq.gz", gzip.compress(good)), ("in.fasta", b">r\nACGT\n")):
        (tmp_path / name).write_bytes(blob)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            _edit_file(engine, OP_FILTER, tmp_path / name, d / "out", Table())
    src = tmp_path / "same.fastq"
    src.write_bytes(good)
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _edit_file(engine, OP_FILTER, src, src, Table())
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _edit_file(engine, OP_FILTER, src, d, Table())  # (a directory)
    assert src.read_bytes() == good and os.listdir(d) == []


# ---- gzip out ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [_BLOCK - 1, _BLOCK, _BLOCK + 1, 3 * _BLOCK - 1, 3 * _BLOCK, 3 * _BLOCK + 1])
def test_gzip_forms_block_borders(engine, tmp_path, total):
    text, _ = _records_of_1k(total)
    plain = _edit(engine, OP_SCRUBB, text, Table())
    assert plain == text and len(plain) == total
    blob = engine.edit_fastq_gzip(OP_SCRUBB, text, [], [], ([0], [], []))
    assert gzip.decompress(blob) == plain and blob == engine.gzip(plain)
    es, gs = engine.edit_fastq_gzip(OP_SCRUBB, text, [], [], ([0], [], []), out_path=str(tmp_path / "o.fastq.gz"))
    assert (tmp_path / "o.fastq.gz").read_bytes() == blob and os.listdir(tmp_path) == ["o.fastq.gz"]
    assert gs["in_bytes"] == total == es["out_bytes"] and gs["out_bytes"] == len(blob) and gs["n_members"] == (total + _BLOCK - 1) // _BLOCK


def test_gzip_forms_on_the_fixture_and_nothing_kept(engine, golden_dir):
    text = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read()
    res, names, lengths, _ = engine.ingest_report(os.path.join(golden_dir, "truth.yacrd"), 0.8)  # (0.8: see test_golden_fixture_all_four_ops)
    for op in OPS:
        truth = gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % OP_NAMES[op]), "rb").read()
        blob = engine.edit_fastq_gzip(op, text, names, lengths, res)
        assert gzip.decompress(blob) == truth and blob == engine.gzip(truth), OP_NAMES[op]
    assert engine.edit_fastq_gzip(OP_EXTRACT, b"@r\nACGT\n+\n!!!!\n", [], [], ([0], [], [])) == _EOF_MEMBER
    assert engine.edit_fastq_gzip(OP_SCRUBB, b"", [], [], ([0], [], [])) == _EOF_MEMBER


# ---- the engine's life --------------------------------------------------------------------------------------------------------
def test_buffers_go_with_trim_and_the_engine():
    before = live_bytes()
    text, table = _filler(3 * TILE) + _TARGET, _TARGET_TABLE
    names, lengths, bo, br, rt = table.arrays()
    with yacrd_amd.Engine(device_id=0) as e:
        e.edit_fastq_text(OP_SCRUBB, text, names, lengths, (bo, br, rt))
        e.edit_fastq_gzip(OP_SCRUBB, text, names, lengths, (bo, br, rt))
        e.trim()
        warm = live_bytes()  # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers)
        for op in OPS:
            e.edit_fastq_text(op, text, names, lengths, (bo, br, rt))
        e.edit_fastq_gzip(OP_SPLIT, text, names, lengths, (bo, br, rt))
        held = live_bytes()
        assert held[0] > warm[0] + len(text) and held[1] >= warm[1] + 2 * _PIECE
        e.trim()
        assert live_bytes() == warm
    assert live_bytes() == before


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


def _inflated(path):
    blob = open(path, "rb").read()
    return gzip.decompress(blob) if blob[:2] == b"\x1f\x8b" else blob


@pytest.mark.parametrize("op", ["scrubb", "filter", "extract", "split"])
@pytest.mark.parametrize("form", ["plain", "gzip1", "bgzf"])
def test_cli_on_the_fixture(golden_dir, tmp_path, op, form):
    text = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read()
    ext = ".fastq" if form == "plain" else ".fastq.gz"
    src = tmp_path / ("reads" + ext)
    src.write_bytes(text if form == "plain" else gzip.compress(text, 1) if form == "gzip1" else host.bgzf_encode_host(text))
    rep = os.path.join(golden_dir, "truth.yacrd")
    a, b = tmp_path / ("dev" + ext), tmp_path / ("host" + ext)
    p = _cli(["-i", rep, "-o", tmp_path / "r.yacrd", "-n", "0.8", op, "-i", src, "-o", a], YACRD_CLI_TIMING="1")
    assert p.returncode == 0, p.stderr
    assert len([l for l in p.stderr.splitlines() if l.startswith("[info] device fastq editor:")]) == 1, p.stderr
    q = _cli(["-i", rep, "-o", tmp_path / "r2.yacrd", "-n", "0.8", op, "-i", src, "-o", b], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_EDITOR="1")
    assert q.returncode == 0 and "[info] device fastq editor" not in q.stderr, q.stderr
    truth = gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % op), "rb").read()
    assert _inflated(a) == _inflated(b) == truth
    if form != "plain":
        assert open(a, "rb").read()[:2] == b"\x1f\x8b"
        r = _cli(["-i", rep, "-o", tmp_path / "r3.yacrd", "-n", "0.8", op, "-i", src, "-o", a], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_DEFLATE="1")
        assert r.returncode == 0 and "[info] device fastq editor" not in r.stderr and _inflated(a) == truth


def test_cli_hands_the_host_what_is_the_hosts(tmp_path):
    rep = tmp_path / "in.yacrd"
    rep.write_text("Chimeric\tok\t10\t2,2,4\nChimeric\tfar\t40\t10,20,30\n")
    good = b"@ok a b\nACGTACGTAC\n+\n!!!!!!!!!!\n"
    for tag, text in (("crlf", good + good.replace(b"\n", b"\r\n") + good), ("beyond", good + b"@far\nACGTACGTACGT\n+\n!!!!!!!!!!!!\n" + good)):
        src = tmp_path / (tag + ".fastq")
        src.write_bytes(text)
        runs = []
        for env in ({"YACRD_NO_DEVICE_EDITOR": "1"}, {}):
            o = tmp_path / ("%s%d.fastq" % (tag, len(runs)))
            p = _cli(["-i", rep, "-o", tmp_path / "again.yacrd", "scrubb", "-i", src, "-o", o], YACRD_CLI_TIMING="1", **env)
            assert "[info] device fastq editor" not in p.stderr
            runs.append((p.returncode, [l for l in p.stderr.splitlines() if l.startswith("[ERROR]")], o.read_bytes()))
        assert runs[0] == runs[1] and runs[0][0] == 0 and runs[0][2].startswith(b"@ok_0_2 a b\nAC\n+\n!!\n@ok_4_10 a b\n")
        assert len(runs[0][1]) == (1 if tag == "beyond" else 0)
