"""BGZF inflated on the GPU (yacrd_engine_gunzip_mem, the editors' _bgzf_ forms; csrc/gpu_inflate.hip, csrc/inflate_block.h).
The yardsticks are Python's zlib and the editors' gzip forms over the inflated text — never the device inflate itself.  The
inputs that must be refused are those tests/test_inflate_cases.py runs through the same decoder text on the CPU, also under
AddressSanitizer and UBSan: what is expected here is a status, not a fault."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import edit_fasta_cases
import edit_fastq_cases
import inflate_cases as ic
import yacrd_amd
from deflate_cases import BLOCK, EOF_MEMBER, fuzz_text
from edit_fastq_cases import OPS, OP_FILTER, OP_NAMES, OP_SCRUBB, SEGMENT, Table
from yacrd_amd import host
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


def _gunzip(engine, blob):
    """the text, or None when the device refuses"""
    try:
        return engine.gunzip(blob)
    except yacrd_amd.NeedsHostParser:
        return None


# ---- gunzip -----------------------------------------------------------------------------------------------------------------------
def test_valid_streams_give_their_text(engine):
    for name, blob, text in ic.valid_cases():
        assert engine.gunzip(blob) == text, name
        st = engine.gunzip_stats
        assert (st["in_bytes"], st["out_bytes"], st["n_members"]) == (len(blob), len(text), len(ic.walk(blob))), name


def test_gunzip_of_gzip_is_the_text(engine):
    for seed in range(60):
        d = fuzz_text(seed)
        assert engine.gunzip(engine.gzip(d)) == d, seed


@pytest.mark.parametrize("n_members", [0, 1, 3, 4, 5, 257, 1031])
def test_member_counts_and_members_that_share_words(engine, n_members):
    """members of 1, 2, 3, 5 ... bytes of text begin at every byte offset of a dword; 1031: more than the device holds at once"""
    r = random.Random(n_members)
    sizes = [(1, 2, 3, 5, 7, 64, 255, 700)[k % 8] for k in range(n_members)]
    parts = [r.randbytes(s) if k % 3 else bytes([65 + k % 26]) * s for k, s in enumerate(sizes)]
    blob = b"".join(ic.member(p, 6) if k % 2 else ic.stored_member(p) for k, p in enumerate(parts))
    assert engine.gunzip(blob) == b"".join(parts)
    assert engine.gunzip_stats["n_members"] == n_members


def test_what_is_not_taken_is_refused_and_the_engine_stays_usable(engine):
    good_blob, good = ic.bgzf_of(fuzz_text(4), level=1), fuzz_text(4)
    for name, blob, _ in ic.not_taken_cases():
        assert _gunzip(engine, blob) is None, name
    for name, blob in ic.not_bgzf_cases():
        assert _gunzip(engine, blob) is None, name
    assert engine.gunzip(good_blob) == good
    taken = 0
    for k, blob in enumerate(ic.mutations(200)):
        got = _gunzip(engine, blob)
        if got is not None:
            taken += 1
            assert got == ic.zlib_says(blob), "mutation %d" % k
    assert 0 < taken < 200
    assert engine.gunzip(good_blob) == good


def test_a_member_across_the_movers_segment_border(engine):
    """a level-0 stream of 128 MiB + 4 MiB of noise: members of 65 280 bytes and their 31 bytes of frame lie across every 4 MiB
    chunk border of the mover and across the 128 MiB segment border of the COMPRESSED stream"""
    try:
        noise = np.random.default_rng(11).integers(0, 256, SEGMENT + (4 << 20), dtype=np.uint8).tobytes()
        blob = ic.bgzf_of(noise, stored=True)
        assert len(blob) > SEGMENT + (4 << 20) and SEGMENT % (BLOCK + 31) != 0  # (the border lies inside a member)
        got = engine.gunzip(blob)
        assert len(got) == len(noise) and got == noise
    finally:
        engine.trim()


# ---- the editors ----------------------------------------------------------------------------------------------------------------
def _reads_fasta(golden_dir):
    lines = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read().split(b"\n")
    return b"".join(b">" + h[1:] + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in zip(lines[0::4], lines[1::4]) if h)


def _both_forms(engine, fmt, op, blob, text, names, lengths, res, tmp_path, tag):
    """the _bgzf_ forms over `blob` against the _gzip_ form over `text`, in memory and into a file"""
    edit_gzip = getattr(engine, "edit_%s_gzip" % fmt)
    edit_bgzf = getattr(engine, "edit_%s_bgzf" % fmt)
    want = edit_gzip(op, text, names, lengths, res)
    assert edit_bgzf(op, blob, names, lengths, res) == want, tag
    us = engine.gunzip_stats
    assert (us["in_bytes"], us["out_bytes"], us["n_members"]) == (len(blob), len(text), len(ic.walk(blob))), tag
    out = tmp_path / "out.gz"
    es, gs = edit_bgzf(op, blob, names, lengths, res, out_path=str(out))
    assert out.read_bytes() == want and es["text_bytes"] == len(text) and gs["out_bytes"] == len(want), tag
    out.unlink()


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_the_fixture_reframed_as_bgzf(engine, golden_dir, tmp_path, fmt):
    text = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read() if fmt == "fastq" else _reads_fasta(golden_dir)
    blob = ic.bgzf_of(text, chunk=60001)
    res, names, lengths, _ = engine.ingest_report(os.path.join(golden_dir, "truth.yacrd"), 0.8)
    for op in OPS:
        _both_forms(engine, fmt, op, blob, text, names, lengths, res, tmp_path, OP_NAMES[op])
        if fmt == "fastq":
            truth = gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % OP_NAMES[op]), "rb").read()
            assert gzip.decompress(engine.edit_fastq_bgzf(op, blob, names, lengths, res)) == truth
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_forty_cases_of_the_editors_fuzz_sets(engine, tmp_path, fmt):
    cases = list((edit_fastq_cases if fmt == "fastq" else edit_fasta_cases).fuzz_cases())
    picked = cases[::max(1, len(cases) // 40)][:40]
    assert len(picked) == 40
    for k, (tag, text, table) in enumerate(picked):
        names, lengths, bo, br, rt = table.arrays()
        blob = ic.bgzf_of(text, chunk=(BLOCK, 777, 65536, 4099)[k % 4], level=(1, 6, 9, 0)[k % 4])
        for op in OPS:
            _both_forms(engine, fmt, op, blob, text, names, lengths, (bo, br, rt), tmp_path, (tag, op))


def _refused(engine, fmt, blob, tmp_path, table=None):
    names, lengths, bo, br, rt = (table or Table()).arrays()
    edit = getattr(engine, "edit_%s_bgzf" % fmt)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(yacrd_amd.NeedsHostParser):
        edit(OP_FILTER, blob, names, lengths, (bo, br, rt))
    with pytest.raises(yacrd_amd.NeedsHostParser):
        edit(OP_SCRUBB, blob, names, lengths, (bo, br, rt), out_path=str(tmp_path / "out.gz"))
    assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_what_the_inflated_text_hides_falls_back(engine, tmp_path, fmt):
    """a CR, and a text without its last newline, inside the inflated text; what is not BGZF; a member not taken"""
    good = b"@r a\nACGT\n+\n!!!!\n" * 5000 if fmt == "fastq" else b">r a\nACGTAC\n" * 5000
    names, lengths, bo, br, rt = Table().arrays()
    assert gzip.decompress(getattr(engine, "edit_%s_bgzf" % fmt)(OP_FILTER, ic.bgzf_of(good), names, lengths, (bo, br, rt))) == good
    (tmp_path / "other").write_bytes(b"what was there")
    _refused(engine, fmt, ic.bgzf_of(good[:70000] + b"\r" + good[70000:]), tmp_path)
    _refused(engine, fmt, ic.bgzf_of(good[:-1]), tmp_path)
    _refused(engine, fmt, gzip.compress(good, 1), tmp_path)
    blob = bytearray(ic.bgzf_of(good))
    blob[len(blob) // 2] ^= 0x10
    assert ic.zlib_says(bytes(blob)) is None
    _refused(engine, fmt, bytes(blob), tmp_path)
    assert (tmp_path / "other").read_bytes() == b"what was there"


def test_a_corrupt_member_behind_the_first_segment_of_text(engine, tmp_path):
    """good records for more than 128 MiB of text, then a member whose CRC does not match: nothing is written"""
    try:
        block = b"@ok a b\nACGTACGTAC\n+\n!!!!!!!!!!\n" * 2040  # 65 280 bytes
        assert len(block) == BLOCK
        m = ic.member(block, 1)
        n = SEGMENT // BLOCK + 40
        bad = bytearray(m)
        bad[-8] ^= 1
        names, lengths, bo, br, rt = Table().arrays()
        good = m * n + EOF_MEMBER
        es, gs = engine.edit_fastq_bgzf(OP_FILTER, good, names, lengths, (bo, br, rt), out_path=str(tmp_path / "good.gz"))
        assert es["text_bytes"] == n * BLOCK == es["out_bytes"] and engine.gunzip_stats["n_members"] == n + 1
        os.remove(tmp_path / "good.gz")
        _refused(engine, "fastq", m * (n - 3) + bytes(bad) + m * 3 + EOF_MEMBER, tmp_path)
    finally:
        engine.trim()


# ---- the engine's life --------------------------------------------------------------------------------------------------------
def test_buffers_go_with_trim_and_the_engine():
    before = live_bytes()
    text = b"@r a\nACGT\n+\n!!!!\n" * 20000
    blob = ic.bgzf_of(text)
    names, lengths, bo, br, rt = Table().arrays()
    with yacrd_amd.Engine(device_id=0) as e:
        e.gunzip(blob)
        e.edit_fastq_bgzf(OP_SCRUBB, blob, names, lengths, (bo, br, rt))
        e.trim()
        warm = live_bytes()  # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers)
        assert e.gunzip(blob) == text
        e.edit_fastq_bgzf(OP_SCRUBB, blob, names, lengths, (bo, br, rt))
        held = live_bytes()
        assert held[0] > warm[0] + len(text) + len(blob) and held[1] > warm[1]
        e.trim()
        assert live_bytes() == warm
    assert live_bytes() == before


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


def _lines(p, head):
    return [l for l in p.stderr.splitlines() if l.startswith(head)]


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("op", ["scrubb", "filter"])
def test_cli_inflates_bgzf_on_the_device(golden_dir, tmp_path, fmt, op):
    """a BGZF FASTQ / FASTA: the bytes of the run under YACRD_NO_DEVICE_INFLATE=1 (the host inflates), and the inflate's line"""
    text = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read() if fmt == "fastq" else _reads_fasta(golden_dir)
    src = tmp_path / ("reads.%s.gz" % fmt)
    src.write_bytes(ic.bgzf_of(text, chunk=50000))
    rep = os.path.join(golden_dir, "truth.yacrd")
    a, b = tmp_path / ("dev.%s.gz" % fmt), tmp_path / ("host.%s.gz" % fmt)
    p = _cli(["-i", rep, "-o", tmp_path / "r.yacrd", "-n", "0.8", op, "-i", src, "-o", a], YACRD_CLI_TIMING="1")
    assert p.returncode == 0, p.stderr
    assert len(_lines(p, "[info] device inflate:")) == 1 and len(_lines(p, "[info] device %s editor:" % fmt)) == 1, p.stderr
    assert (" %d -> %d bytes" % (os.path.getsize(src), len(text))) in _lines(p, "[info] device inflate:")[0]
    q = _cli(["-i", rep, "-o", tmp_path / "r2.yacrd", "-n", "0.8", op, "-i", src, "-o", b], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_INFLATE="1")
    assert q.returncode == 0 and not _lines(q, "[info] device inflate:") and len(_lines(q, "[info] device %s editor:" % fmt)) == 1, q.stderr
    assert a.read_bytes() == b.read_bytes() and len(gzip.decompress(a.read_bytes())) > 0
    if fmt == "fastq":
        assert gzip.decompress(a.read_bytes()) == gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % op), "rb").read()


def test_cli_leaves_plain_gzip_to_the_host(golden_dir, tmp_path):
    text = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read()
    src = tmp_path / "reads.fastq.gz"
    src.write_bytes(gzip.compress(text, 1))
    rep = os.path.join(golden_dir, "truth.yacrd")
    a, b = tmp_path / "dev.fastq.gz", tmp_path / "host.fastq.gz"
    p = _cli(["-i", rep, "-o", tmp_path / "r.yacrd", "-n", "0.8", "scrubb", "-i", src, "-o", a], YACRD_CLI_TIMING="1")
    q = _cli(["-i", rep, "-o", tmp_path / "r2.yacrd", "-n", "0.8", "scrubb", "-i", src, "-o", b], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_INFLATE="1")
    assert p.returncode == 0 and q.returncode == 0, p.stderr + q.stderr
    assert not _lines(p, "[info] device inflate:") and len(_lines(p, "[info] device fastq editor:")) == 1, p.stderr
    assert a.read_bytes() == b.read_bytes()
    assert gzip.decompress(a.read_bytes()) == gzip.open(os.path.join(golden_dir, "truth.scrubb.fastq.gz"), "rb").read()
