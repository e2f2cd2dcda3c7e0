"""scrubb / split / filter / extract on FASTA on the GPU (yacrd_engine_edit_fasta, csrc/gpu_seq_edit.hip).  The yardsticks for
bytes are the host loop (yacrd_edit_file on a ".fasta": host.edit_file, or the CLI under YACRD_NO_DEVICE_EDITOR=1) and the
restatement that tests/test_edit_fasta_cases.py pins to it on the CPU — never the device path itself."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import edit_fastq_cases as fq
import yacrd_amd
from edit_fasta_cases import (BASES_FIRST, CHIMERIC, NOT_COVERED, OPS, OP_EXTRACT, OP_FILTER, OP_SCRUBB, OP_SPLIT, Table, _regions, fallback_cases,
                              fuzz_cases, host_loop, lay_out, restate)
from edit_fastq_cases import OUT_TILE, SEGMENT, TILE
from test_editors import OPS as OP_BY_NAME, UNIT, table_from_reads
from yacrd_amd import host
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
_PIECE = 4 << 20   # what one trip home of the output carries (csrc/gpu_seq_edit.hip: kOutPiece)
_BLOCK = 65280     # bytes of text per BGZF member (csrc/bgzf_sizes.h: kBlock)
_EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_NO_TABLE = ([], [], ([0], [], []))


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


def _edit(engine, op, text, table):
    names, lengths, bo, br, rt = table.arrays()
    return engine.edit_fasta_text(op, text, names, lengths, (bo, br, rt))


def _edit_file(engine, op, src, out, table):
    names, lengths, bo, br, rt = table.arrays()
    return engine.edit_fasta(op, str(src), str(out), names, lengths, (bo, br, rt))


def _both(engine, tmp_path, op, text, table):
    """the device's bytes, checked against the restatement and the host loop"""
    got = _edit(engine, op, text, table)
    want, n_in, n_out = restate(text, op, table)
    assert got == want, (op, len(text))
    assert got == host_loop(str(tmp_path), op, text, table, ext=".fasta"), (op, len(text))
    st = engine.seq_edit_stats
    assert (st["text_bytes"], st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(text), len(want), n_in, n_out)
    return got


# ---- the reference's vectors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,data,reads,expect", [(u[0], u[2], u[3], u[4]) for u in UNIT if u[1] == ".fasta"])
def test_reference_editor_unit_vectors(engine, op, data, reads, expect):
    names, lengths, bo, br, rt = table_from_reads(reads, 0, 0.8)
    assert engine.edit_fasta_text(OP_BY_NAME[op], data, names, lengths, (bo, br, rt)) == expect


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
            assert got == host_loop(str(tmp_path), op, text, table, ext=".fasta"), (tag, op)
            st = engine.seq_edit_stats
            assert (st["text_bytes"], st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(text), len(want), n_in, n_out), (tag, op)
        n += 1
    assert n >= 150


# ---- one pipeline, two formats ---------------------------------------------------------------------------------------------------
def _fastq_records(out):
    lines = out.split(b"\n")
    return [(lines[i][1:].partition(b" ")[0], lines[i][1:].partition(b" ")[2], lines[i + 1]) for i in range(0, len(lines) - 1, 4)]


def _fasta_records(out):
    recs = []
    for chunk in out.split(b">")[1:]:
        head, _, body = chunk.partition(b"\n")
        recs.append((head.partition(b" ")[0], head.partition(b" ")[2], body.replace(b"\n", b"")))
    return recs


@pytest.fixture(scope="module")
def same_reads():
    """260 reads of 1 to 400 bases (the plan crosses a workgroup), their table — types as the oracle derives them from the regions —,
    the reads as FASTQ, and what a FASTA of them is laid out from"""
    import oracle
    rng = random.Random(20250117)
    heads, seqs, quals, names, lens, regs = [], [], [], [], [], []
    for i in range(260):
        n = rng.randint(1, 400)
        name = b"r%d" % i + bytes(rng.choice(b"abcXYZ.:|/-") for _ in range(rng.randint(0, 12)))  # (no '_': a cut piece's name is no read's)
        heads.append(name + (b" " + fq._token(rng, rng.randint(1, 30)) if rng.random() < 0.5 else b""))
        seqs.append(fq._bases(rng, n)), quals.append(fq._quals(rng, n))
        if rng.random() < 0.75:  # (else: absent from the table)
            names.append(name), lens.append(n), regs.append(fq._regions(rng, rng.choice(fq._SHAPES), n))
    table = Table(names, lens, regs, [oracle.type_of_read(l, r, 0.4) for l, r in zip(lens, regs)])
    fastq = b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in zip(heads, seqs, quals))
    return heads, seqs, table, fastq


@pytest.mark.parametrize("width", [80, "ragged"])
def test_fastq_and_fasta_of_the_same_reads_agree(engine, same_reads, width):
    """the two instantiations of the shared plan and copy kernels, on the same reads and the same table: the same output
    records under the same names with the same bases, for all four ops; input lines of 80 bases (the closed form) and ragged
    ones (the search).  Each output is what the restatement of its format says, and what oracle/editors.py says"""
    from oracle import editors as oracle_editors
    heads, seqs, table, fastq = same_reads
    rng = random.Random(5)
    fasta = b"".join(b">" + h + b"\n" + lay_out(rng, s, width) for h, s in zip(heads, seqs))
    names, lengths, bo, br, rt = table.arrays()
    ot = fq.oracle_table(table)
    assert ot is not None
    read_names = {h.partition(b" ")[0] for h in heads}
    n_cut = 0
    for op in OPS:
        got_q = engine.edit_fastq_text(op, fastq, names, lengths, (bo, br, rt))
        got_a = engine.edit_fasta_text(op, fasta, names, lengths, (bo, br, rt))
        want_q = oracle_editors.edit_fastq(fq.OP_NAMES[op], fastq, ot, 0.4)
        assert got_q == want_q and got_q == fq.restate(fastq, op, table)[0], op
        assert got_a == restate(fasta, op, table)[0], op
        rq, ra, ro = _fastq_records(got_q), _fasta_records(got_a), _fastq_records(want_q)
        assert len(rq) > 20, op
        assert [r[0] for r in ra] == [r[0] for r in rq] == [r[0] for r in ro], op
        assert [r[2] for r in ra] == [r[2] for r in rq] == [r[2] for r in ro], op
        copied = [k for k, r in enumerate(rq) if r[0] in read_names]
        assert [ra[k][1] for k in copied] == [rq[k][1] for k in copied] == [ro[k][1] for k in copied], op  # (a cut FASTA piece drops it)
        n_cut += len(rq) - len(copied)
    assert n_cut > 100


# ---- rows and words: every length against every input width -------------------------------------------------------------------
_ROW_LENGTHS = [0, 1, 79, 80, 81, 159, 160, 161, 162]
_IN_WIDTHS = [1, 2, 3, 79, 80, 81, None]


def _seq(n, salt=0):
    return bytes(b"ACGT"[(i * 7 + i // 5 + salt) % 4] for i in range(n))


def _blank_behind_the_first_line(lines):
    """a record of one width is addressed without the line tables; a blank line behind its first line makes it one that is
    searched, with the same bases on the same lines"""
    head, nl, rest = lines.partition(b"\n")
    return head + nl + (b"\n" if nl else b"") + rest


@pytest.mark.parametrize("searched", [False, True], ids=["one_width", "searched"])
@pytest.mark.parametrize("width", _IN_WIDTHS, ids=lambda w: "w%s" % w)
def test_lengths_against_an_input_width(engine, tmp_path, width, searched):
    """output rows one base short of, at and one base over a row's end, from input lines of 1 to 3 bases (an output word
    crosses one, two and three input newlines), of 79 to 81 and from one line; copied whole and as cut pieces that begin at
    bases 0, 1, 79, 80 and 81; by the closed form for records of one width and by the search"""
    rng = random.Random(7)
    lay = (lambda r, q, w: _blank_behind_the_first_line(lay_out(r, q, w))) if searched else lay_out
    recs, names, lens, regs = [], [], [], []
    for n in _ROW_LENGTHS:
        recs.append(b">c%d whole\n" % n + lay(rng, _seq(n, n), width))
        for p0 in (0, 1, 79, 80, 81):
            name, total = b"p%d_%d" % (n, p0), p0 + n + 5
            recs.append(b">" + name + b"\tcut\n" + lay(rng, _seq(total, p0), width))
            names.append(name), lens.append(total), regs.append([(0, p0), (p0 + n, total)])  # scrubb: the piece [p0, p0 + n)
    text, table = b"".join(recs), Table(names, lens, regs, [CHIMERIC] * len(names))
    got = _both(engine, tmp_path, OP_SCRUBB, text, table)
    assert b">p162_81_81_243\n" in got and b">p0_79_79_79\n>" in got
    for op in (OP_FILTER, OP_EXTRACT, OP_SPLIT):
        _both(engine, tmp_path, op, text, table)


def test_records_of_one_width_and_nearly(engine, tmp_path):
    """what decides between the closed form and the search: the last line as long as the others, shorter, one base, longer by
    one; a first line that differs; a blank line at the end, in the middle; two lines, one line; a thousand lines, one of
    which differs, so that the line which decides is another workgroup's than the record's first"""
    shapes = [[7, 7, 7], [7, 7, 6], [7, 7, 1], [7, 7, 8], [6, 7, 7], [8, 7, 7], [7, 7, 0], [7, 0, 7], [7, 8], [8, 7], [7, 7], [7], [0, 7], [7, 6, 7, 6],
              [3] * 40 + [2], [3] * 40 + [4], [90] * 3 + [89], [90, 91, 90],
              [3] * 1000 + [2], [3] * 700 + [4] + [3] * 300, [3] * 700 + [0] + [3] * 300]  # the line that differs far from the first
    recs, names, lens, regs = [], [], [], []
    for i, shape in enumerate(shapes):
        seq, at = _seq(sum(shape), i), 0
        recs.append(b">s%d\n" % i)
        for k in shape:
            recs.append(seq[at:at + k] + b"\n")
            at += k
        names.append(b"s%d" % i), lens.append(len(seq)), regs.append([(2, 3), (len(seq) - 2, len(seq) - 1)])
    text, table = b"".join(recs), Table(names, lens, regs, [CHIMERIC] * len(names))
    for op in OPS:
        _both(engine, tmp_path, op, text, table)


def test_ragged_and_blank_lines(engine, tmp_path):
    text = (b"\n\n>a one\nAC\n\nGT\n\n\n>empty followed by a header\n>b\n\nACGTACGT\n" + b"A" * 90 + b"\n\nC\n>last\nAC\n\n\n")
    table = Table([b"a", b"b", b"empty"], [4, 99, 0], [[(1, 2)], [(3, 95)], []], [CHIMERIC, CHIMERIC, CHIMERIC])
    for op in OPS:
        _both(engine, tmp_path, op, text, table)
    assert _edit(engine, OP_SCRUBB, text, table) == (b">a_0_1\nA\n>a_2_4\nGT\n>empty followed by a header\n>b_0_3\nACG\n>b_95_99\nAAAC\n>last\nAC\n")
    assert _edit(engine, OP_SCRUBB, b"", Table()) == b"" and engine.seq_edit_stats["n_records"] == 0
    assert _edit(engine, OP_FILTER, b"\n\n\n", Table()) == b"" and engine.seq_edit_stats["n_records"] == 0


def test_separators_and_descriptions(engine, tmp_path):
    text = (b">r \nAC\n>r\t\nAC\n>r\x0c\nAC\n>r\td\nAC\n>r\x0cd\nAC\n>r d\nAC\n>r  two blanks\nAC\n>r a >b\t c \nAC\n>r \t\nAC\n")
    want = b">r\nAC\n>r\nAC\n>r\nAC\n>r d\nAC\n>r d\nAC\n>r d\nAC\n>r  two blanks\nAC\n>r a >b\t c \nAC\n>r \t\nAC\n"
    assert _both(engine, tmp_path, OP_FILTER, text, Table()) == want
    cut = Table([b"r"], [2], [[(1, 2)]], [CHIMERIC])
    assert _both(engine, tmp_path, OP_SCRUBB, text, cut) == b">r_0_1\nA\n" * 9  # a cut piece loses its description
    _both(engine, tmp_path, OP_SPLIT, text, cut)


def test_ids_prefixes_and_lengths(engine, tmp_path):
    long_id = b"L" * 300
    table = Table([b"a", b"ab", long_id], [4, 4, 4], [[(0, 1)], [(1, 2)], [(2, 3)]], [CHIMERIC, CHIMERIC, NOT_COVERED])
    text = b">a\nACGT\n>ab\nACGT\n>abc\nACGT\n>" + long_id + b" d\nACGT\n>" + long_id[:299] + b"\nACGT\n>a\tb\nACGT\n"
    for op in OPS:
        _both(engine, tmp_path, op, text, table)
    assert _edit(engine, OP_SCRUBB, text, table) == b">a_1_4\nCGT\n>ab_0_1\nA\n>ab_2_4\nGT\n>abc\nACGT\n>" + long_id[:299] + b"\nACGT\n>a_1_4\nCGT\n"


# ---- text tile borders -----------------------------------------------------------------------------------------------------------
def _filler(size):
    """records `>f`, absent from every table and written back as they stand, of exactly `size` bytes (3, or 5 and more)"""
    parts = []
    while size:
        take = 84 if size == 84 or size >= 89 else size - 5 if size > 84 else size
        assert take == 3 or 5 <= take <= 84, size
        parts.append(b">f\n" + (b"G" * (take - 4) + b"\n" if take > 3 else b""))
        size -= take
    return b"".join(parts)


_TARGET = b">target of the cut\n" + b"ACGT" * 5 + b"\n" + b"TTGCA" * 4 + b"\n"
_TARGET_TABLE = Table([b"target"], [40], [[(5, 10), (20, 21)]], [CHIMERIC])


@pytest.mark.parametrize("tiles", [1, 2, 3])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_text_of_whole_tiles_and_a_byte(engine, tmp_path, tiles, d):
    """the text's last newline lies before, on and behind a tile border"""
    text = _filler(tiles * TILE + d - len(_TARGET)) + _TARGET
    assert len(text) == tiles * TILE + d
    for op in (OP_SCRUBB, OP_FILTER):
        _both(engine, tmp_path, op, text, _TARGET_TABLE)


@pytest.mark.parametrize("what,before", [("mark_first_of_a_tile", 0), ("mark_last_of_a_tile", 1), ("header", 3),
                                          ("header_newline", len(b">target of the cut")), ("first_base", 19), ("sequence_line", 30),
                                          ("between_lines", 40), ("last_newline", len(_TARGET) - 1)])
def test_a_line_straddles_a_tile_border(engine, tmp_path, what, before):
    """byte `before` of the cut record is the first of the second tile"""
    text = _filler(TILE - before) + _TARGET + _filler(100)
    assert text[TILE - before:].startswith(_TARGET)
    for op in OPS:
        _both(engine, tmp_path, op, text, _TARGET_TABLE)


def test_many_short_lines_and_records(engine, tmp_path):
    """~300 000 lines of 1 to 3 bases in ~1 000 records: the scans over the lines and the plan cross workgroups"""
    rng = random.Random(11)
    gen = np.random.default_rng(11)
    recs, names, lens, regs, types = [], [], [], [], []
    for r in range(1000):
        n = rng.randint(500, 700)
        seq = bytes(np.frombuffer(b"ACGT", np.uint8)[gen.integers(0, 4, n)])
        cuts = np.cumsum(gen.integers(1, 4, n))
        cuts = cuts[cuts < n].tolist()
        recs.append(b">r%d x\n" % r + b"".join(seq[a:b] + b"\n" for a, b in zip([0] + cuts, cuts + [n])))
        if r % 3:
            names.append(b"r%d" % r), lens.append(n), regs.append(_regions(rng, "many" if r % 2 else "middle", n)), types.append(r % 3 - 1 + r % 2)
    text = b"".join(recs)
    assert text.count(b"\n") > 290000
    table = Table(names, lens, regs, types)
    for op in OPS:
        _both(engine, tmp_path, op, text, table)


@pytest.mark.parametrize("width", [None, 60, "ragged"])
def test_a_record_of_100000_bases(engine, tmp_path, width):
    rng = random.Random(3)
    n = 100000
    seq = bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(3).integers(0, 4, n)])
    text = _filler(1001) + b">long one\n" + lay_out(rng, seq, width) + _filler(77)
    assert text.count(b"\n") > (1667 if width else 1)
    table = Table([b"long"], [n], [_regions(rng, "many", n)], [CHIMERIC])
    for op in OPS:
        _both(engine, tmp_path, op, text, table)
    edges = Table([b"long"], [n], [[(0, 7), (32768, 65536), (65536, 65537), (99999, 100000)]], [CHIMERIC])
    _both(engine, tmp_path, OP_SCRUBB, text, edges)


# ---- output borders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_output_of_whole_tiles_and_a_byte(engine, k, d):
    """everything is copied: the output ends one byte before, on and one byte behind an output tile border"""
    text = _filler(k * OUT_TILE + d)
    assert _edit(engine, OP_SCRUBB, text, _TARGET_TABLE) == text and engine.seq_edit_stats["out_bytes"] == k * OUT_TILE + d


@pytest.mark.parametrize("at", [OUT_TILE - 1, OUT_TILE])
def test_a_rows_newline_at_an_output_tile_border(engine, tmp_path, at):
    """the first row's newline of a 200-base record is the last byte of the first output tile, and the first of the second"""
    text = _filler(at - 83) + b">t\n" + _seq(200) + b"\n"
    got = _both(engine, tmp_path, OP_FILTER, text, Table())
    assert got[at:at + 1] == b"\n" and got[at - 80:at] == _seq(200)[:80] and got[at + 1:at + 81] == _seq(200)[80:160]


@pytest.mark.parametrize("before", [1, 3, 8, 11, 12, 13])
def test_a_cut_header_straddles_an_output_tile_border(engine, tmp_path, before):
    """the copied records in front fill the first output tile but `before` bytes: `>target_0_5` lies across the border"""
    text = _filler(OUT_TILE - before) + _TARGET
    for op in (OP_SCRUBB, OP_SPLIT):
        got = _both(engine, tmp_path, op, text, _TARGET_TABLE)
        assert got[OUT_TILE - before:].startswith(b">target_0_5\nACGTA\n>target_10_20\n")


@pytest.mark.parametrize("total", [_PIECE - 1, _PIECE, _PIECE + 1, 2 * _PIECE + 1])
def test_piece_borders_of_the_way_home(engine, tmp_path, total):
    """everything is kept: the output ends one byte before, on and one byte behind a piece border of the way home, and behind
    two pieces — out of memory, into a file and through the encoder"""
    text = _filler(total)
    assert len(text) == total
    assert _edit(engine, OP_FILTER, text, Table()) == text and engine.seq_edit_stats["out_bytes"] == total
    src, out = tmp_path / "in.fasta", tmp_path / "out.fasta"
    src.write_bytes(text)
    st = _edit_file(engine, OP_SCRUBB, src, out, Table())
    assert out.read_bytes() == text and st["out_bytes"] == total and st["n_records"] == st["n_out_records"] == text.count(b">")
    assert gzip.decompress(engine.edit_fasta_gzip(OP_FILTER, text, *_NO_TABLE)) == text
    assert engine.gzip_stats["in_bytes"] == total
    assert sorted(os.listdir(tmp_path)) == ["in.fasta", "out.fasta"]


# ---- the segment border ---------------------------------------------------------------------------------------------------------
def _streams_equal(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 22), fb.read(1 << 22)
            if x != y:
                return False
            if not x:
                return True


_OK = b">ok a b\nACGTAC\nGTAC\n"


@pytest.fixture(scope="module")
def big_prefix():
    """good records, `ok` cut under scrubb, up to 6 bytes short of the mover's first segment border"""
    block = (_OK + _filler(1003)) * 1024
    reps = (SEGMENT - 6) // len(block) - 1
    body = block * reps
    return body + _filler(SEGMENT - 6 - len(body))


def test_records_across_the_segment_border(engine, big_prefix):
    """a text just over 128 MiB + 4 MiB: a cut record whose header lies in front of the segment border and whose lines lie
    behind it; against the host loop, compared in streams"""
    d = "/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp"
    tag = os.path.join(d, "yacrd_fasta_edit_test_%d_" % os.getpid())
    n = 1000
    wide = b">wide\n" + lay_out(random.Random(1), _seq(n), 70)
    tail = (_OK + _filler(1003)) * (4 * 1024 + 7)
    text = big_prefix + wide + tail
    assert len(big_prefix) == SEGMENT - 6 and text[SEGMENT:SEGMENT + 4] == _seq(4) and SEGMENT + (4 << 20) < len(text) < SEGMENT + (5 << 20)
    table = Table([b"ok", b"wide"], [10, n], [[(2, 4)], [(100, 150), (400, 600)]], [CHIMERIC, CHIMERIC])
    names, lengths, bo, br, rt = table.arrays()
    src, want, got = tag + "in.fasta", tag + "host.fasta", tag + "dev.fasta"
    try:
        with open(src, "wb") as f:
            f.write(text)
        host.edit_file(OP_SCRUBB, src, want, names, lengths, bo, br, rt)
        st = engine.edit_fasta(OP_SCRUBB, src, got, names, lengths, (bo, br, rt))
        assert _streams_equal(want, got)
        assert st["out_bytes"] == os.path.getsize(want) and st["text_bytes"] == len(text) and st["n_out_records"] > st["n_records"]
    finally:
        for x in (src, want, got):
            if os.path.exists(x):
                os.remove(x)
        engine.trim()


# ---- what falls back ----------------------------------------------------------------------------------------------------------------
_FALLBACKS = fallback_cases() + [("bases_first_%d" % i, OPS, t, Table()) for i, t in enumerate(BASES_FIRST)]
_BEHIND = {tag: _filler(TILE + 100) + text for tag, _, text, _ in fallback_cases()}
_BEHIND.update(("bases_first_%d" % i, b"\n" * (TILE + 5) + t) for i, t in enumerate(BASES_FIRST))  # (blank lines may stand in front)


@pytest.mark.parametrize("where", ["first_tile", "behind_the_border"])
@pytest.mark.parametrize("tag,ops,text,table", _FALLBACKS, ids=[f[0] for f in _FALLBACKS])
def test_what_must_fall_back_does_and_writes_nothing(engine, tmp_path, tag, ops, text, table, where):
    if where == "behind_the_border":
        text = _BEHIND[tag]
    d = tmp_path / "dev"
    d.mkdir()
    src, out = tmp_path / "in.fasta", d / "out.fasta"
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
    assert os.listdir(d) == ["out.fasta"] and out.read_bytes() == b"what was there"
    with pytest.raises(yacrd_amd.NeedsHostParser):
        names, lengths, bo, br, rt = table.arrays()
        engine.edit_fasta_gzip(ops[0], text, names, lengths, (bo, br, rt), out_path=str(d / "out.fasta.gz"))
    assert os.listdir(d) == ["out.fasta"] and src.read_bytes() == text
    for op in set(OPS) - set(ops):  # (a cut position is nothing to filter and extract)
        _both(engine, tmp_path, op, text, table)


def test_other_inputs_of_the_file_form_fall_back(engine, tmp_path):
    good = b">r\nACGT\n"
    d = tmp_path / "dev"
    d.mkdir()
    for name, blob in (("in.fasta.gz", gzip.compress(good)), ("in.fastq", good), ("in.fa.fq", good), ("in.paf.fa", good), ("in.txt", good)):
        (tmp_path / name).write_bytes(blob)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            _edit_file(engine, OP_FILTER, tmp_path / name, d / "out", Table())
    src = tmp_path / "same.fa"
    src.write_bytes(good)
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _edit_file(engine, OP_FILTER, src, src, Table())
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _edit_file(engine, OP_FILTER, src, d, Table())  # (a directory)
    assert src.read_bytes() == good and os.listdir(d) == []
    _edit_file(engine, OP_FILTER, src, d / "out.fa", Table())  # (".fa" is a FASTA's name)
    assert (d / "out.fa").read_bytes() == good and os.listdir(d) == ["out.fa"]


# ---- gzip out ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [_BLOCK - 1, _BLOCK, _BLOCK + 1, 3 * _BLOCK - 1, 3 * _BLOCK, 3 * _BLOCK + 1])
def test_gzip_forms_block_borders(engine, tmp_path, total):
    text = _filler(total)
    plain = _edit(engine, OP_FILTER, text, Table())
    assert plain == text and len(plain) == total
    blob = engine.edit_fasta_gzip(OP_FILTER, text, *_NO_TABLE)
    assert gzip.decompress(blob) == plain and blob == engine.gzip(plain)
    es, gs = engine.edit_fasta_gzip(OP_FILTER, text, *_NO_TABLE, out_path=str(tmp_path / "o.fasta.gz"))
    assert (tmp_path / "o.fasta.gz").read_bytes() == blob and os.listdir(tmp_path) == ["o.fasta.gz"]
    assert gs["in_bytes"] == total == es["out_bytes"] and gs["out_bytes"] == len(blob) and gs["n_members"] == (total + _BLOCK - 1) // _BLOCK


def test_gzip_forms_cut_and_nothing_kept(engine, tmp_path):
    text = _filler(3 * TILE) + _TARGET
    names, lengths, bo, br, rt = _TARGET_TABLE.arrays()
    for op in OPS:
        want = restate(text, op, _TARGET_TABLE)[0]
        assert want == host_loop(str(tmp_path), op, text, _TARGET_TABLE, ext=".fasta")
        blob = engine.edit_fasta_gzip(op, text, names, lengths, (bo, br, rt))
        assert gzip.decompress(blob) == want and blob == engine.gzip(want), op
    assert engine.edit_fasta_gzip(OP_EXTRACT, b">r\nACGT\n", *_NO_TABLE) == _EOF_MEMBER
    assert engine.edit_fasta_gzip(OP_SCRUBB, b"", *_NO_TABLE) == _EOF_MEMBER
    assert engine.edit_fasta_gzip(OP_SCRUBB, b"\n\n", *_NO_TABLE) == _EOF_MEMBER


# ---- the engine's life --------------------------------------------------------------------------------------------------------
def test_buffers_go_with_trim_and_the_engine():
    before = live_bytes()
    text, table = _filler(3 * TILE) + _TARGET, _TARGET_TABLE
    names, lengths, bo, br, rt = table.arrays()
    with yacrd_amd.Engine(device_id=0) as e:
        e.edit_fasta_text(OP_SCRUBB, text, names, lengths, (bo, br, rt))
        e.edit_fasta_gzip(OP_SCRUBB, text, names, lengths, (bo, br, rt))
        e.trim()
        warm = live_bytes()  # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers)
        for op in OPS:
            e.edit_fasta_text(op, text, names, lengths, (bo, br, rt))
        e.edit_fasta_gzip(OP_SPLIT, text, names, lengths, (bo, br, rt))
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


@pytest.fixture(scope="module")
def reads_fasta(golden_dir):
    """tests/golden/reads.fastq.gz as FASTA, 60 bases a line"""
    lines = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read().split(b"\n")
    return b"".join(b">" + h[1:] + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in zip(lines[0::4], lines[1::4]) if h)


@pytest.mark.parametrize("op", ["scrubb", "filter", "extract", "split"])
@pytest.mark.parametrize("form", ["plain", "gzip1", "bgzf"])
def test_cli_on_the_fixture(golden_dir, reads_fasta, tmp_path, op, form):
    ext = ".fasta" if form == "plain" else ".fasta.gz"
    src = tmp_path / ("reads" + ext)
    src.write_bytes(reads_fasta if form == "plain" else gzip.compress(reads_fasta, 1) if form == "gzip1" else host.bgzf_encode_host(reads_fasta))
    rep = os.path.join(golden_dir, "truth.yacrd")
    a, b = tmp_path / ("dev" + ext), tmp_path / ("host" + ext)
    p = _cli(["-i", rep, "-o", tmp_path / "r.yacrd", "-n", "0.8", op, "-i", src, "-o", a], YACRD_CLI_TIMING="1")
    assert p.returncode == 0, p.stderr
    assert len([l for l in p.stderr.splitlines() if l.startswith("[info] device fasta editor:")]) == 1, p.stderr
    assert "[info] device fastq editor" not in p.stderr
    q = _cli(["-i", rep, "-o", tmp_path / "r2.yacrd", "-n", "0.8", op, "-i", src, "-o", b], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_EDITOR="1")
    assert q.returncode == 0 and "[info] device fasta editor" not in q.stderr, q.stderr
    assert _inflated(a) == _inflated(b) and len(_inflated(b)) > 0 and _inflated(b).count(b">") == gzip.open(
        os.path.join(golden_dir, "truth.%s.fastq.gz" % op), "rb").read().count(b"\n") // 4
    if form != "plain":
        assert open(a, "rb").read()[:2] == b"\x1f\x8b"
        r = _cli(["-i", rep, "-o", tmp_path / "r3.yacrd", "-n", "0.8", op, "-i", src, "-o", a], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_DEFLATE="1")
        assert r.returncode == 0 and "[info] device fasta editor" not in r.stderr and _inflated(a) == _inflated(b)


def test_cli_hands_the_host_what_is_the_hosts(tmp_path):
    rep = tmp_path / "in.yacrd"
    rep.write_text("Chimeric\tok\t10\t2,2,4\nChimeric\tfar\t40\t10,20,30\n")
    good = b">ok a b\nACGTAC\nGTAC\n"
    for tag, text in (("crlf", good + good.replace(b"\n", b"\r\n") + good), ("beyond", good + b">far\nACGTACGTACGT\n" + good)):
        src = tmp_path / (tag + ".fasta")
        src.write_bytes(text)
        runs = []
        for env in ({"YACRD_NO_DEVICE_EDITOR": "1"}, {}):
            o = tmp_path / ("%s%d.fasta" % (tag, len(runs)))
            p = _cli(["-i", rep, "-o", tmp_path / "again.yacrd", "scrubb", "-i", src, "-o", o], YACRD_CLI_TIMING="1", **env)
            assert "[info] device fasta editor" not in p.stderr
            runs.append((p.returncode, [l for l in p.stderr.splitlines() if l.startswith("[ERROR]")], o.read_bytes()))
        assert runs[0] == runs[1] and runs[0][0] == 0 and runs[0][2].startswith(b">ok_0_2\nAC\n>ok_4_10\nACGTAC\n")
        assert len(runs[0][1]) == (1 if tag == "beyond" else 0)
