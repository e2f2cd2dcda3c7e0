"""Plain gzip inflated on the GPU (yacrd_engine_gunzip_stream_mem; csrc/gpu_gunzip_stream.hip, csrc/inflate_stream.h).  The
yardstick is Python's zlib — never the device decoder itself — and, for the counters, the same decoder text run by one host
thread at the same chunk size.  The inputs that must be refused are those tests/test_gunzip_stream_cases.py runs through
the same text on the CPU, also under AddressSanitizer and UBSan: what is expected here is a status, not a fault."""
import gzip
import os
import subprocess

import pytest

import edit_fasta_cases
import edit_fastq_cases
import gunzip_stream_cases as gc
import inflate_cases as ic
import yacrd_amd
from deflate_cases import fuzz_text
from edit_fastq_cases import OPS, OP_FILTER, OP_NAMES, OP_SCRUBB, Table
from yacrd_amd import host
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")

COUNTERS = ("n_chunks", "n_spans", "n_false_starts", "rounds", "n_blocks", "out_bytes")
CHUNKS = (1024, 4096, 0)  # 0: the default


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e
        e.debug_gunzip_chunk(0)


def _gunzip(engine, blob):
    """the text, or None when the device refuses"""
    try:
        return engine.gunzip_stream(blob)
    except yacrd_amd.NeedsHostParser:
        return None


def test_the_symbols_are_exported():
    assert "yacrd_engine_gunzip_stream_mem" in yacrd_amd.EXPORTED_SYMBOLS and "yacrd_debug_gunzip_chunk" in yacrd_amd.DEBUG_SYMBOLS


@pytest.mark.parametrize("chunk", CHUNKS)
def test_valid_streams_give_zlibs_bytes_and_the_host_builds_counters(engine, chunk):
    engine.debug_gunzip_chunk(chunk)
    for name, blob, text in gc.valid_cases():
        assert engine.gunzip_stream(blob) == text, (name, chunk)
        st = engine.gunzip_stream_stats
        want = host.gzip_stream_decode_host(blob, chunk)[1]
        assert {k: st[k] for k in COUNTERS} == want, (name, chunk)
        assert st["in_bytes"] == len(blob) and st["n_spans"] >= 1 + gc.chunks_with_a_start(blob, chunk or 32768), (name, chunk)
    engine.debug_gunzip_chunk(0)


def test_the_chunk_has_a_floor(engine):
    with pytest.raises(yacrd_amd.EngineError):
        engine.debug_gunzip_chunk(1023)


def test_what_is_not_taken_is_refused_and_the_engine_stays_usable(engine):
    name, good_blob, good = gc.valid_cases()[0]
    for chunk in (1024, 0):
        engine.debug_gunzip_chunk(chunk)
        for name, blob, cause in gc.refused_cases():
            with pytest.raises(yacrd_amd.NeedsHostParser) as e:
                engine.gunzip_stream(blob)
            if cause:
                assert cause in str(e.value), (name, str(e.value))
            assert engine.gunzip_stream(good_blob) == good, name  # (right after every refusal)


def test_mutations_are_refused_or_zlibs_bytes(engine):
    taken = 0
    for k, blob in enumerate(gc.mutations(200)):
        engine.debug_gunzip_chunk((1024, 4096, 0)[k % 3])
        got = _gunzip(engine, blob)
        if got is not None:
            taken += 1
            assert got == gc.zlib_says(blob), "mutation %d" % k
    engine.debug_gunzip_chunk(0)
    assert 0 < taken < 200
    name, good_blob, good = gc.valid_cases()[0]
    assert engine.gunzip_stream(good_blob) == good


def test_gunzip_of_gzip_compress_is_the_text(engine):
    for seed in range(40):
        d = fuzz_text(seed)
        engine.debug_gunzip_chunk((1024, 0)[seed % 2])
        assert engine.gunzip_stream(gzip.compress(d, (1, 6, 9)[seed % 3])) == d, seed
    engine.debug_gunzip_chunk(0)


# ---- the editors ----------------------------------------------------------------------------------------------------------------
def _reads_fasta(golden_dir):
    lines = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read().split(b"\n")
    return b"".join(b">" + h[1:] + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in zip(lines[0::4], lines[1::4]) if h)


def _both_forms(engine, fmt, op, blob, text, names, lengths, res, tmp_path, tag):
    """the _gz_ forms over `blob` against the _gzip_ form over `text`, in memory and into a file"""
    want = getattr(engine, "edit_%s_gzip" % fmt)(op, text, names, lengths, res)
    edit_gz = getattr(engine, "edit_%s_gz" % fmt)
    assert edit_gz(op, blob, names, lengths, res) == want, tag
    zs = engine.gunzip_stream_stats
    assert (zs["in_bytes"], zs["out_bytes"]) == (len(blob), len(text)) and zs["n_spans"] >= 1, tag
    out = tmp_path / "out.gz"
    es, gs = edit_gz(op, blob, names, lengths, res, out_path=str(out))
    assert out.read_bytes() == want and es["text_bytes"] == len(text) and gs["out_bytes"] == len(want), tag
    out.unlink()


def test_the_fixture_is_plain_gzip():
    blob = open(os.path.join(ROOT, "tests", "golden", "reads.fastq.gz"), "rb").read()
    assert blob[3] == 0 and ic.walk(blob) is None and len(gc.zlib_says(blob)) == 1059085


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_the_fixture_as_it_lies_in_the_repository(engine, golden_dir, tmp_path, fmt):
    raw = open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read()
    text = gzip.decompress(raw) if fmt == "fastq" else _reads_fasta(golden_dir)
    blob = raw if fmt == "fastq" else gzip.compress(text, 6)
    res, names, lengths, _ = engine.ingest_report(os.path.join(golden_dir, "truth.yacrd"), 0.8)
    for k, op in enumerate(OPS):
        engine.debug_gunzip_chunk((1024, 4096, 0, 0)[k % 4])
        _both_forms(engine, fmt, op, blob, text, names, lengths, res, tmp_path, OP_NAMES[op])
        if fmt == "fastq":
            truth = gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % OP_NAMES[op]), "rb").read()
            assert gzip.decompress(engine.edit_fastq_gz(op, blob, names, lengths, res)) == truth
    engine.debug_gunzip_chunk(0)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_twenty_cases_of_the_editors_fuzz_sets(engine, tmp_path, fmt):
    cases = list((edit_fastq_cases if fmt == "fastq" else edit_fasta_cases).fuzz_cases())
    picked = cases[::max(1, len(cases) // 20)][:20]
    assert len(picked) == 20
    for k, (tag, text, table) in enumerate(picked):
        names, lengths, bo, br, rt = table.arrays()
        blob = gzip.compress(text, (1, 6, 9, 0)[k % 4])
        engine.debug_gunzip_chunk((1024, 0)[k % 2])
        for op in OPS:
            _both_forms(engine, fmt, op, blob, text, names, lengths, (bo, br, rt), tmp_path, (tag, op))
    engine.debug_gunzip_chunk(0)


def _refused(engine, fmt, blob, tmp_path):
    names, lengths, bo, br, rt = Table().arrays()
    edit = getattr(engine, "edit_%s_gz" % fmt)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(yacrd_amd.NeedsHostParser):
        edit(OP_FILTER, blob, names, lengths, (bo, br, rt))
    with pytest.raises(yacrd_amd.NeedsHostParser):
        edit(OP_SCRUBB, blob, names, lengths, (bo, br, rt), out_path=str(tmp_path / "out.gz"))
    assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_what_the_inflated_text_hides_falls_back(engine, tmp_path, fmt):
    """a CR, and a text without its last newline, inside the inflated text; a damaged payload; BGZF; a text beyond the window"""
    good = b"@r a\nACGT\n+\n!!!!\n" * 5000 if fmt == "fastq" else b">r a\nACGTAC\n" * 5000
    names, lengths, bo, br, rt = Table().arrays()
    assert gzip.decompress(getattr(engine, "edit_%s_gz" % fmt)(OP_FILTER, gzip.compress(good), names, lengths, (bo, br, rt))) == good
    (tmp_path / "other").write_bytes(b"what was there")
    _refused(engine, fmt, gzip.compress(good[:70000] + b"\r" + good[70000:]), tmp_path)
    _refused(engine, fmt, gzip.compress(good[:-1]), tmp_path)
    _refused(engine, fmt, ic.bgzf_of(good), tmp_path)
    blob = bytearray(gzip.compress(good, 1))
    blob[len(blob) // 2] ^= 0x10
    assert gc.zlib_says(bytes(blob)) is None
    _refused(engine, fmt, bytes(blob), tmp_path)
    engine.debug_seq_window(32768)  # (the text is longer: the run would go in windows)
    try:
        _refused(engine, fmt, gzip.compress(good), tmp_path)
    finally:
        engine.debug_seq_window(0)
    assert (tmp_path / "other").read_bytes() == b"what was there"


# ---- the engine's life --------------------------------------------------------------------------------------------------------
def test_buffers_go_with_trim_and_the_engine():
    before = live_bytes()
    name, blob, text = gc.valid_cases()[0]
    fq = b"@r a\nACGT\n+\n!!!!\n" * 20000
    names, lengths, bo, br, rt = Table().arrays()
    with yacrd_amd.Engine(device_id=0) as e:
        e.gunzip_stream(blob)
        e.edit_fastq_gz(OP_SCRUBB, gzip.compress(fq), names, lengths, (bo, br, rt))
        e.trim()
        warm = live_bytes()  # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers)
        assert e.gunzip_stream(blob) == text
        e.edit_fastq_gz(OP_SCRUBB, gzip.compress(fq), names, lengths, (bo, br, rt))
        held = live_bytes()
        assert held[0] > warm[0] + 3 * len(text) + len(blob) and held[1] > warm[1]
        e.trim()
        assert live_bytes() == warm
    assert live_bytes() == before


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


def _lines(p, head):
    return [l for l in p.stderr.splitlines() if l.startswith(head)]


@pytest.mark.parametrize("op", ["scrubb", "filter"])
def test_cli_takes_the_device_route_only_when_asked(golden_dir, tmp_path, op):
    """the fixture, a plain gzip FASTQ: the same output file with YACRD_DEVICE_GUNZIP=1 and without; the route's line with it,
    none without it or under YACRD_NO_DEVICE_INFLATE=1"""
    src = os.path.join(golden_dir, "reads.fastq.gz")
    rep = os.path.join(golden_dir, "truth.yacrd")
    outs = []
    for k, env in enumerate(({"YACRD_DEVICE_GUNZIP": "1"}, {}, {"YACRD_DEVICE_GUNZIP": "1", "YACRD_NO_DEVICE_INFLATE": "1"})):
        out = tmp_path / ("out%d.fastq.gz" % k)
        p = _cli(["-i", rep, "-o", tmp_path / ("r%d.yacrd" % k), "-n", "0.8", op, "-i", src, "-o", out], YACRD_CLI_TIMING="1", **env)
        assert p.returncode == 0, p.stderr
        assert len(_lines(p, "[info] device gunzip:")) == (1 if k == 0 else 0), p.stderr
        assert len(_lines(p, "[info] device fastq editor:")) == 1 and not _lines(p, "[info] device inflate:"), p.stderr
        if k == 0:
            assert (" %d -> 1059085 bytes" % os.path.getsize(src)) in _lines(p, "[info] device gunzip:")[0]
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] == outs[2]
    assert gzip.decompress(outs[0]) == gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % op), "rb").read()
