"""Device deflate: Engine.gzip / GzipWriter / the CLI's gzip output.  The reference is zlib (Python's zlib / gzip and
`gzip -t`), never the encoder's own decoder; the bytes are also compared with the same text run by one host thread."""
import gzip
import hashlib
import os
import random
import shutil
import subprocess

import pytest

import yacrd_amd
from yacrd_amd import host

from deflate_cases import BLOCK, EOF_MEMBER, fastq_like, fuzz_text, huffman_only_size, paf_like, walk_bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


@pytest.fixture(scope="module")
def golden_fastq(golden_dir):
    return gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read()


def check(engine, data, host_too=True):
    blob = engine.gzip(data)
    assert gzip.decompress(blob) == data
    members = walk_bgzf(blob)
    n_members = (len(data) + BLOCK - 1) // BLOCK
    assert members[-1][0] == EOF_MEMBER and len(members) - 1 == n_members
    st = engine.gzip_stats
    assert (st["in_bytes"], st["out_bytes"], st["n_members"]) == (len(data), len(blob), n_members)
    if len(data) >= BLOCK:
        assert len(blob) <= 1.02 * huffman_only_size(data) + 28
    assert len(blob) <= len(data) + 31 * n_members + 28
    if host_too:
        assert blob == host.bgzf_encode_host(data), "the device's bytes are the host-compiled encoder's"
    return blob


def corpus(golden_dir, golden_fastq, tmp_path_factory):
    r = random.Random(11)
    yield "empty", b""
    yield "one byte", b"x"
    for n in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):
        yield "noise %d" % n, r.randbytes(n)
    yield "zeros", bytes(1 << 20)
    yield "one byte repeated", b"\xa7" * (1 << 20)
    for period in range(2, 301):
        yield "period %d" % period, (r.randbytes(period) * (70000 // period + 1))[:70000]
    yield "all byte values", bytes(range(256)) * 4096
    yield "4 MiB of noise", random.Random(12).randbytes(4 << 20)
    yield "golden fastq", golden_fastq
    yield "golden paf", open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    p = str(tmp_path_factory.mktemp("synth") / "s.fastq")
    host.synth_fastq(host.SYNTH_ONT, 300, 3000, 7, 10, p)
    yield "synthetic fastq", open(p, "rb").read()
    yield "no final newline", b"@r1\nACGT\n+\n????\n@r2\nAC" * 9000 + b"GT"


def test_round_trip_and_container(engine, golden_dir, golden_fastq, tmp_path_factory):
    d = tmp_path_factory.mktemp("rt")
    for name, data in corpus(golden_dir, golden_fastq, tmp_path_factory):
        blob = check(engine, data)
        f = d / "x.gz"
        f.write_bytes(blob)
        assert subprocess.run(["gzip", "-t", str(f)]).returncode == 0, name
        if len(data) > BLOCK:
            with host.text_from_file(str(f)) as t:
                assert t.members > 1 and t.bytes() == data, name


def test_stored_members(engine):
    data = random.Random(2).randbytes(3 * BLOCK)
    check(engine, data)
    assert engine.gzip_stats["n_stored"] == 3


def test_matches_are_found(engine, golden_dir):
    r = random.Random(6)
    for data in [open(os.path.join(golden_dir, "reads.paf"), "rb").read(), fastq_like(r, 900, const_quality=True), bytes(1 << 20)]:
        assert len(check(engine, data)) < huffman_only_size(data)


def test_fuzz(engine):
    for seed in range(1000):
        check(engine, fuzz_text(seed), host_too=seed % 4 == 0)


def through_writer(engine, data, path, seg, slices):
    r = random.Random(len(data) * 31 + seg)
    with engine.gzip_writer(str(path), segment_bytes=seg) as w:
        at = 0
        while at < len(data):
            k = r.choice(slices)
            w.write(data[at:at + k])
            at += k
    assert w.stats["in_bytes"] == len(data) and w.stats["n_members"] == (len(data) + BLOCK - 1) // BLOCK
    return path.read_bytes()


def test_fuzz_segment_boundaries(engine, tmp_path):
    """The fuzz texts whose lengths sit on and around 1, 2 and 4 blocks, through the writer with segments of one and of two
    blocks: texts that end exactly on a segment boundary (the last segment is full), one byte short of it and one beyond."""
    out = tmp_path / "f.gz"
    n_on_boundary = 0
    for seed in range(1000):
        if seed % 3 == 0:
            continue  # (lengths drawn at random: test_fuzz)
        data = fuzz_text(seed)
        for seg in (BLOCK, 2 * BLOCK):
            blob = through_writer(engine, data, out, seg, [1, 255, 4096, 65279, 65280, 65281, 200000])
            assert gzip.decompress(blob) == data, (seed, seg)
            walk_bgzf(blob)
            if seed % 8 == 1:
                assert blob == engine.gzip(data), (seed, seg)
            n_on_boundary += len(data) > 0 and len(data) % seg == 0
    assert n_on_boundary >= 20, "the fuzz reaches full last segments"


@pytest.mark.parametrize("seg_blocks", [1, 2, 3])
def test_texts_that_end_on_a_segment(engine, tmp_path, seg_blocks):
    seg = seg_blocks * BLOCK
    base = fastq_like(random.Random(seg_blocks), 3 * seg // 250 + 400)
    assert len(base) > 3 * seg + 1
    for n in (seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, 2 * seg + 1, 3 * seg):
        data = base[:n]
        for slices in ([n], [seg], [BLOCK], [1000, 65279]):
            blob = through_writer(engine, data, tmp_path / "s.gz", seg, slices)
            assert gzip.decompress(blob) == data and blob == engine.gzip(data), (n, slices)
            assert walk_bgzf(blob)[-1][0] == EOF_MEMBER


def test_determinism_and_segments(engine, golden_fastq, tmp_path):
    data = golden_fastq * 3 + b"tail"
    first = engine.gzip(data)
    assert engine.gzip(data) == first
    r = random.Random(9)
    for seg in (BLOCK, 5 * BLOCK + 17, 0):
        out = tmp_path / ("w%d.gz" % seg)
        with engine.gzip_writer(str(out), segment_bytes=seg) as w:
            at = 0
            while at < len(data):
                k = r.choice([1, 7, 4095, 65279, 65281, 300001])
                w.write(data[at:at + k])
                at += k
        assert out.read_bytes() == first, "segment_bytes %d" % seg
        assert w.stats["in_bytes"] == len(data) and w.stats["out_bytes"] == len(first)
        assert not [n for n in os.listdir(tmp_path) if ".gz." in n], "close leaves exactly out_path"


def test_writer_files(engine, tmp_path):
    with pytest.raises(yacrd_amd.EngineError):
        engine.gzip_writer(str(tmp_path / "no_such_dir" / "x.gz"))
    assert os.listdir(tmp_path) == []
    w = engine.gzip_writer(str(tmp_path / "a.gz"))
    w.write(b"abc" * 100000)
    w.abort()
    assert os.listdir(tmp_path) == []
    with pytest.raises(RuntimeError):
        with engine.gzip_writer(str(tmp_path / "b.gz")) as w:
            w.write(b"abc")
            raise RuntimeError("the edit failed")
    assert os.listdir(tmp_path) == []
    with engine.gzip_writer(str(tmp_path / "c.gz")) as w:
        w.write(b"abc")
    assert os.listdir(tmp_path) == ["c.gz"] and gzip.decompress((tmp_path / "c.gz").read_bytes()) == b"abc"
    with engine.gzip_writer(str(tmp_path / "c.gz")):
        pass
    assert (tmp_path / "c.gz").read_bytes() == EOF_MEMBER


def test_sink_into_writer(engine, golden_dir, tmp_path):
    import numpy as np
    import oracle
    with open(os.path.join(golden_dir, "reads.paf")) as f:
        names, offsets, intervals, lengths = oracle.to_csr(oracle.parse_paf(f))
    bo, br, rt = oracle.run(offsets, intervals, lengths, 0, 0.8)
    out = tmp_path / "scrubbed.fastq.gz"
    with engine.gzip_writer(str(out)) as w:
        host.edit_file_to(host.OP_SCRUBB, os.path.join(golden_dir, "reads.fastq.gz"), w.sink(), names, lengths.astype(np.uint32), bo, br, rt)
    assert gzip.decompress(out.read_bytes()) == gzip.open(os.path.join(golden_dir, "truth.scrubb.fastq.gz"), "rb").read()


# ---- the CLI ----------------------------------------------------------------------------------------------------------
def cli(*args, env=None):
    p = subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def is_bgzf(blob):
    return blob[:4] == b"\x1f\x8b\x08\x04" and blob[12:14] == b"BC" and blob.endswith(EOF_MEMBER)


@pytest.mark.parametrize("op", ["scrubb", "filter", "extract", "split"])
def test_cli_gzip_in_bgzf_out(golden_dir, tmp_path, op):
    shutil.copy(os.path.join(golden_dir, "reads.fastq.gz"), tmp_path / "reads.fastq.gz")
    paf = os.path.join(golden_dir, "reads.paf")
    truth = gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % op), "rb").read()
    out = tmp_path / "out.fastq.gz"
    p = cli("-i", paf, "-o", str(tmp_path / "r.yacrd"), op, "-i", str(tmp_path / "reads.fastq.gz"), "-o", str(out), env={"YACRD_CLI_TIMING": "1"})
    blob = out.read_bytes()
    assert gzip.decompress(blob) == truth and is_bgzf(blob)
    walk_bgzf(blob)
    assert "[info] device deflate:" in p.stderr
    old = tmp_path / "old.fastq.gz"
    cli("-i", paf, "-o", str(tmp_path / "r.yacrd"), op, "-i", str(tmp_path / "reads.fastq.gz"), "-o", str(old), env={"YACRD_NO_DEVICE_DEFLATE": "1"})
    blob = old.read_bytes()
    assert gzip.decompress(blob) == truth and not is_bgzf(blob) and blob[3] == 0, "one zlib stream, as before"
    assert sorted(os.listdir(tmp_path)) == ["old.fastq.gz", "out.fastq.gz", "r.yacrd", "reads.fastq.gz"]


def test_cli_other_compressions_and_overlaps(golden_dir, golden_fastq, tmp_path):
    import bz2
    import lzma
    paf = os.path.join(golden_dir, "reads.paf")
    truth = gzip.open(os.path.join(golden_dir, "truth.scrubb.fastq.gz"), "rb").read()
    for ext, mod, magic in ((".bz2", bz2, b"BZh"), (".xz", lzma, b"\xfd7zXZ")):
        src = tmp_path / ("reads.fastq" + ext)
        src.write_bytes(mod.compress(golden_fastq))
        out = tmp_path / ("out.fastq" + ext)
        cli("-i", paf, "-o", str(tmp_path / "r.yacrd"), "scrubb", "-i", str(src), "-o", str(out))
        assert out.read_bytes().startswith(magic) and mod.decompress(out.read_bytes()) == truth
    gz = tmp_path / "reads.paf.gz"
    gz.write_bytes(gzip.compress(open(paf, "rb").read()))
    cli("-i", paf, "-o", str(tmp_path / "r.yacrd"), "filter", "-i", str(gz), "-o", str(tmp_path / "f.paf.gz"))
    cli("-i", paf, "-o", str(tmp_path / "r.yacrd"), "filter", "-i", paf, "-o", str(tmp_path / "f.paf"), env={"YACRD_NO_DEVICE_EDITOR": "1"})
    blob = (tmp_path / "f.paf.gz").read_bytes()
    assert is_bgzf(blob) and gzip.decompress(blob) == (tmp_path / "f.paf").read_bytes()


def test_one_gib_through_the_writer(engine, tmp_path):
    """About 1 GiB of synthetic FASTQ through the writer, inflated member-parallel by the project's own reader."""
    piece = fastq_like(random.Random(21), 40000)  # about 20 MB
    rounds = (1 << 30) // len(piece) + 1
    h = hashlib.sha256()
    out = tmp_path / "big.fastq.gz"
    with engine.gzip_writer(str(out)) as w:
        for i in range(rounds):
            chunk = b"@round%d\n" % i + piece
            h.update(chunk)
            w.write(chunk)
    st = w.stats
    print("1 GiB writer: %d -> %d bytes, kernels %.1f ms (%.2f GB/s), h2d %.1f ms, d2h %.1f ms, write %.1f ms" % (
        st["in_bytes"], st["out_bytes"], st["kernel_ms"], st["in_bytes"] / 1e6 / max(st["kernel_ms"], 1e-3), st["h2d_ms"], st["d2h_ms"], st["write_ms"]))
    with host.text_from_file(str(out)) as t:
        assert t.members > 1 and t.n_bytes == st["in_bytes"]
        import ctypes
        assert hashlib.sha256((ctypes.c_char * t.n_bytes).from_address(t.address)).hexdigest() == h.hexdigest()
