"""filter / extract on gzip overlap files with the kept bytes deflated on the GPU (yacrd_engine_edit_overlaps_gzip_mem / _file,
csrc/gpu_edit.hip + csrc/gpu_deflate.hip).  Every comparison is exact.  The yardsticks: for the kept bytes the host loop
(yacrd_edit_file) and the ten-line restatement; for the members the host build of the encoder (deflate_host.cc over
deflate_block.h) and Engine.gzip on the kept bytes; zlib and walk_bgzf for the container."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import yacrd_amd
from deflate_cases import BLOCK, EOF_MEMBER, walk_bgzf
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, fuzz_cases, host_loop, restate
from edit_overlaps_gzip_cases import seam_text
from yacrd_amd import host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
SEGMENT = 128 << 20  # csrc/gpu_text.h: kTextChunk * kTextSeg

# the reference's unit vectors (src/editor/filter.rs:289-359, extract.rs:293-362) and their three reads, read 1 bad
_PAF_UNIT = (b"1\t12000\t20\t4500\t-\t2\t10000\t5500\t10000\t4500\t4500\t255\n"
             b"1\t12000\t5500\t10000\t-\t3\t10000\t0\t4500\t4500\t4500\t255\n")
_M4_UNIT = b"1 2 0.1 2 0 100 450 1000 0 550 900 1000\n1 3 0.1 2 0 550 900 1000 0 100 450 1000\n"
_UNIT_NAMES, _UNIT_TYPES = [b"1", b"2", b"3"], [yacrd_amd.NOT_COVERED, yacrd_amd.NOT_BAD, yacrd_amd.NOT_BAD]


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


def _well_formed(blob, kept):
    """members of at most 65 280 bytes of text, cut at multiples of it from the start of the kept stream, EOF_MEMBER last"""
    members = walk_bgzf(blob)
    assert members[-1][0] == EOF_MEMBER
    sizes = [len(d) for _, d in members[:-1]]
    assert sizes == [BLOCK] * (len(kept) // BLOCK) + ([len(kept) % BLOCK] if len(kept) % BLOCK else [])
    assert b"".join(d for _, d in members) == kept


def _check(engine, op, text, names, types, fmt, kept, host_encoder=True):
    blob = engine.edit_overlaps_gzip(op, text, names, types, fmt)  # (raises on YACRD_EFALLBACK)
    es, gs = engine.edit_stats, engine.gzip_stats
    assert gzip.decompress(blob) == kept
    assert blob == engine.gzip(kept)
    if host_encoder:
        assert blob == host.bgzf_encode_host(kept)
    _well_formed(blob, kept)
    assert es["kept_bytes"] == len(kept) == gs["in_bytes"] and es["text_bytes"] == len(text)
    assert gs["out_bytes"] == len(blob) and gs["n_members"] == (len(kept) + BLOCK - 1) // BLOCK
    return blob


# ---- 1. unit vectors, fixture, fuzz -------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [OP_FILTER, OP_EXTRACT])
@pytest.mark.parametrize("fmt,text", [(1, _PAF_UNIT), (2, _M4_UNIT)])
def test_reference_unit_vectors(engine, tmp_path, op, fmt, text):
    table = dict(zip(_UNIT_NAMES, _UNIT_TYPES))
    more = text + (b"2\t1000\t0\t500\t+\t3\t1000\t500\t1000\t500\t500\t255\n" if fmt == 1 else b"2 3 0.1 2 0 0 500 1000 0 500 1000 1000\n")
    for t in (text, more):
        kept = restate(t, op, table, fmt == 2)[0]
        assert kept == host_loop(str(tmp_path), op, t, _UNIT_NAMES, _UNIT_TYPES, ".paf" if fmt == 1 else ".m4")
        _check(engine, op, t, _UNIT_NAMES, _UNIT_TYPES, fmt, kept)
    # every line of the vectors names read 1: filter drops them all, extract keeps them all
    assert gzip.decompress(engine.edit_overlaps_gzip(op, text, _UNIT_NAMES, _UNIT_TYPES, fmt)) == (b"" if op == OP_FILTER else text)


@pytest.mark.parametrize("cov,ncov", [(0, 0.8), (4, 0.4)])
def test_fixture_with_two_detections(engine, golden_dir, tmp_path, cov, ncov):
    paf = os.path.join(golden_dir, "reads.paf")
    res, names, lengths, _ = engine.ingest_paf(paf, cov, ncov)
    text = open(paf, "rb").read()
    table = dict(zip([n.encode() for n in names], res.read_type.tolist()))
    for op in (OP_FILTER, OP_EXTRACT):
        want = str(tmp_path / "host.paf")
        host.edit_file(op, paf, want, names, lengths, res.bad_offsets, res.bad_regions, res.read_type, n_threads=1)
        kept = open(want, "rb").read()
        assert kept == restate(text, op, table, False)[0] and 0 < len(kept) < len(text)
        _check(engine, op, text, names, res.read_type, 1, kept)
        # the file form: the same bytes at out_path, nothing beside it
        d = tmp_path / ("out%d" % op)
        d.mkdir()
        es, gs = engine.edit_overlaps_gzip(op, text, names, res.read_type, 1, out_path=str(d / "k.paf.gz"))
        assert os.listdir(d) == ["k.paf.gz"] and (d / "k.paf.gz").read_bytes() == engine.gzip(kept)
        assert es["kept_bytes"] == gs["in_bytes"] == len(kept)


def test_fuzz_zero_fallbacks(engine, tmp_path):
    """every text of the fuzz set is taken (no NeedsHostParser), the kept bytes are the host loop's and the restatement's,
    the members those of Engine.gzip and of the encoder's host build"""
    n = 0
    for tag, text, m4, names, types in fuzz_cases():
        table = dict(zip(names, types))
        for op in (OP_FILTER, OP_EXTRACT):
            kept, n_lines, n_kept = restate(text, op, table, m4)
            assert kept == host_loop(str(tmp_path), op, text, names, types, ".m4" if m4 else ".paf"), (tag, m4, op)
            _check(engine, op, text, names, types, 2 if m4 else 1, kept)
            assert (engine.edit_stats["n_kept"], engine.edit_stats["n_lines"]) == (n_kept, n_lines), (tag, m4, op)
        n += 1
    assert n >= 1000


# ---- 2. block and segment seams -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [OP_FILTER, OP_EXTRACT])
@pytest.mark.parametrize("m4", [False, True])
def test_block_seams(engine, op, m4):
    rng = random.Random(20241108 + op + 2 * m4)
    for k in (1, 2, 3, 5):
        for d in (-1, 0, 1):
            text, names, types = seam_text(rng, op, m4, k * BLOCK + d)
            plain = engine.edit_overlaps_text(op, text, names, types, 2 if m4 else 1)
            assert len(plain) == k * BLOCK + d and plain == restate(text, op, dict(zip(names, types)), m4)[0]
            _check(engine, op, text, names, types, 2 if m4 else 1, plain)


@pytest.fixture(scope="module")
def synth():
    d = "/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp"
    tag = os.path.join(d, "yacrd_edit_gz_test_%d_" % os.getpid())
    paf = tag + "s.paf"
    host.synth_paf(host.SYNTH_SEQUEL, 50_000, 5_000_000, 20241108 + 5, paf)
    made = [paf]
    yield paf, tag, made
    for x in made:
        if os.path.exists(x):
            os.remove(x)


def test_a_block_straddles_every_segment_border(synth):
    """a PAF longer than two editor segments: whatever is kept, blocks of the kept stream straddle the segments' borders"""
    paf, tag, made = synth
    assert os.path.getsize(paf) > 2 * SEGMENT
    with yacrd_amd.Engine(device_id=0) as e:
        res, names, lengths, _ = e.ingest_paf(paf, 3, 0.4)
        types = res.read_type
        assert (types == 1).sum() > 500 and (types == 2).sum() > 500
        text = np.fromfile(paf, dtype=np.uint8)
        for op in (OP_FILTER, OP_EXTRACT):
            plain = e.edit_overlaps_text(op, text.tobytes(), names, types, 1)
            assert 0 < len(plain) < text.size
            blob = e.edit_overlaps_gzip(op, text, names, types, 1)
            es, gs = e.edit_stats, e.gzip_stats
            print("op %d: %d -> %d kept -> %d bytes, edit %s, gzip %s" % (op, text.size, len(plain), len(blob), es, gs))
            assert blob == e.gzip(plain)
            assert es["kept_bytes"] == gs["in_bytes"] == len(plain) and gs["n_members"] == (len(plain) + BLOCK - 1) // BLOCK
            # the file form, and once more into warm buffers: the bytes do not depend on the run
            out = tag + "k%d.paf.gz" % op
            made.append(out)
            e.edit_overlaps_gzip(op, text, names, types, 1, out_path=out)
            with open(out, "rb") as f:
                assert f.read() == blob
            assert e.edit_overlaps_gzip(op, text, names, types, 1) == blob
            del blob, plain
        e.trim()
        assert e.edit_overlaps_gzip(OP_EXTRACT, _PAF_UNIT, _UNIT_NAMES, _UNIT_TYPES, 1) == e.gzip(_PAF_UNIT)  # (after trim: fresh buffers)


# ---- 3. nothing kept ------------------------------------------------------------------------------------------------------
def test_nothing_kept(engine, tmp_path):
    rng = random.Random(3)
    text, names, _ = seam_text(rng, OP_FILTER, False, 3 * BLOCK)
    types = [0] * len(names)  # every read NotBad: extract keeps nothing
    empty = engine.gzip(b"")
    assert empty == EOF_MEMBER
    for t in (text, b"", b"\n\n"):
        assert engine.edit_overlaps_gzip(OP_EXTRACT, t, names, types, 1) == empty
        assert engine.edit_stats["kept_bytes"] == 0 == engine.gzip_stats["in_bytes"] and engine.gzip_stats["n_members"] == 0
        out = tmp_path / "none.paf.gz"
        engine.edit_overlaps_gzip(OP_EXTRACT, t, names, types, 1, out_path=str(out))
        assert os.listdir(tmp_path) == ["none.paf.gz"] and out.read_bytes() == empty
        out.unlink()


# ---- 4. fallbacks ---------------------------------------------------------------------------------------------------------
_GOOD = b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\t255\n"
_ODD = [
    ("quote", b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\t\"x\"\n"),
    ("cr", b"a\t10\t0\t5\t+\tb\t10\t0\r5\t5\t5\t255\n"),
    ("short_line", b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\n"),
]


@pytest.mark.parametrize("where", ["first_segment", "behind_128MiB"])
@pytest.mark.parametrize("tag,odd", _ODD, ids=[t for t, _ in _ODD])
def test_what_must_fall_back_does_and_leaves_nothing(engine, tmp_path, tag, odd, where):
    lead = 3 if where == "first_segment" else SEGMENT // len(_GOOD) + 1000
    text = _GOOD * lead + odd + _GOOD * 2
    assert (len(_GOOD) * lead > SEGMENT) == (where == "behind_128MiB")
    # read b is bad: extract keeps every line, members of the first segment are on their way when the odd line is met
    for op in (OP_EXTRACT, OP_FILTER):
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps_gzip(op, text, [b"a", b"b"], [0, 1], 1)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps_gzip(op, text, [b"a", b"b"], [0, 1], 1, out_path=str(tmp_path / "out.paf.gz"))
        assert os.listdir(tmp_path) == [], "no file and no temporary beside out_path"
        # the engine's next call works
        assert engine.edit_overlaps_gzip(OP_EXTRACT, _GOOD * 5, [b"a", b"b"], [0, 1], 1) == engine.gzip(_GOOD * 5)


# ---- 5. the CLI -----------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


def _new_path_line(p):
    hit = [l for l in p.stdout.splitlines() if l.startswith("[info] device editor + deflate:")]  # (this one line is on stdout)
    assert len(hit) == 1, p.stdout + p.stderr
    return hit[0]


def _paf_to_m4(text):
    out = []
    for l in text.decode().split("\n"):
        f = l.split("\t")
        out.append(" ".join([f[0], f[5], "0.1", "2", "0", f[2], f[3], f[1], "1", f[7], f[8], f[6]]) if l else l)
    return "\n".join(out).encode()


@pytest.mark.parametrize("op", ["filter", "extract"])
@pytest.mark.parametrize("way", ["gzip", "bgzf", "other_file", "m4"])
def test_cli(engine, golden_dir, tmp_path, op, way):
    text = open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    ext = ".m4" if way == "m4" else ".paf"
    if way == "m4":
        text = _paf_to_m4(text)
    plain = tmp_path / ("x" + ext)
    plain.write_bytes(text)
    x = tmp_path / ("x" + ext + ".gz")
    x.write_bytes(engine.gzip(text) if way == "bgzf" else gzip.compress(text, 1))
    sub_in = x
    if way == "other_file":
        sub_in = tmp_path / "copy.paf.gz"
        sub_in.write_bytes(gzip.compress(text, 6))
    det = ["-c", "4", "-n", "0.4"]
    y, y_host, y_plain = tmp_path / ("y" + ext + ".gz"), tmp_path / ("y_host" + ext + ".gz"), tmp_path / ("y" + ext)
    p = _cli(["-i", x, "-o", tmp_path / "r.yacrd"] + det + [op, "-i", sub_in, "-o", y], YACRD_CLI_TIMING="1")
    assert p.returncode == 0, p.stderr
    line = _new_path_line(p)
    assert ("text_reused=1" if sub_in == x else "text_reused=0") in line
    assert "[info] device deflate:" not in p.stderr, "the host loop did not run"
    q = _cli(["-i", x, "-o", tmp_path / "r2.yacrd"] + det + [op, "-i", sub_in, "-o", y_host], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_EDITOR="1")
    assert q.returncode == 0 and "[info] device editor" not in q.stderr + q.stdout and "[info] device deflate:" in q.stderr
    r = _cli(["-i", plain, "-o", tmp_path / "r3.yacrd"] + det + [op, "-i", plain, "-o", y_plain], YACRD_NO_DEVICE_EDITOR="1")
    assert r.returncode == 0, r.stderr
    blob, kept = y.read_bytes(), y_plain.read_bytes()
    assert blob == y_host.read_bytes(), "byte-identical to the host loop into the gzip writer"
    assert gzip.decompress(blob) == kept and 0 < len(kept) < len(text)
    assert blob == engine.gzip(kept)
    _well_formed(blob, kept)
    assert (tmp_path / "r.yacrd").read_bytes() == (tmp_path / "r2.yacrd").read_bytes() == (tmp_path / "r3.yacrd").read_bytes()
    # YACRD_NO_DEVICE_DEFLATE=1: today's path down to zlib, one stream
    z = tmp_path / ("z" + ext + ".gz")
    s = _cli(["-i", x, "-o", tmp_path / "r4.yacrd"] + det + [op, "-i", sub_in, "-o", z], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_DEFLATE="1")
    assert s.returncode == 0 and "[info] device editor" not in s.stderr + s.stdout and "[info] device deflate" not in s.stderr
    assert gzip.decompress(z.read_bytes()) == kept and z.read_bytes()[3] == 0
    assert sorted(n for n in os.listdir(tmp_path) if n.startswith(("y", "z"))) == sorted(f.name for f in (y, y_host, y_plain, z))


@pytest.mark.parametrize("op", ["filter", "extract"])
def test_cli_quoted_field_and_other_codecs(golden_dir, tmp_path, op):
    import bz2
    import lzma
    text = open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    det = ["-c", "4", "-n", "0.4"]
    # a quoted field: the host path's bytes, by the host path
    lines = text.split(b"\n")
    lines[700] = lines[700] + b"\t\"cg:Z:5M\""
    quoted = b"\n".join(l if i == 700 or not l else l + b"\tcg:Z:5M" for i, l in enumerate(lines))
    x = tmp_path / "q.paf.gz"
    x.write_bytes(gzip.compress(quoted, 1))
    runs = []
    for env in ({"YACRD_NO_DEVICE_EDITOR": "1"}, {}):
        o = tmp_path / ("q%d.paf.gz" % len(runs))
        p = _cli(["-i", x, "-o", tmp_path / "q.yacrd"] + det + [op, "-i", x, "-o", o], YACRD_CLI_TIMING="1", **env)
        assert "[info] device editor" not in p.stderr + p.stdout
        runs.append((p.returncode, [l for l in p.stderr.splitlines() if l.startswith("Error")], o.read_bytes() if o.exists() else None))
    assert runs[0] == runs[1] and runs[0][0] == 0 and runs[0][2] is not None
    assert not [n for n in os.listdir(tmp_path) if ".gz." in n], "no temporary is left"
    # bzip2 / xz: what they were (the host path, the input's codec)
    plain = tmp_path / "p.paf"
    plain.write_bytes(text)
    r = _cli(["-i", plain, "-o", tmp_path / "p.yacrd"] + det + [op, "-i", plain, "-o", tmp_path / "kept.paf"], YACRD_NO_DEVICE_EDITOR="1")
    assert r.returncode == 0, r.stderr
    for ext, mod, magic in ((".bz2", bz2, b"BZh"), (".xz", lzma, b"\xfd7zXZ")):
        src, outs = tmp_path / ("c.paf" + ext), []
        src.write_bytes(mod.compress(text))
        for env in ({"YACRD_NO_DEVICE_EDITOR": "1"}, {}):
            o = tmp_path / ("c%d.paf%s" % (len(outs), ext))
            p = _cli(["-i", src, "-o", tmp_path / "c.yacrd"] + det + [op, "-i", src, "-o", o], YACRD_CLI_TIMING="1", **env)
            assert p.returncode == 0 and "[info] device editor" not in p.stderr + p.stdout, p.stderr
            outs.append(o.read_bytes())
        assert outs[0] == outs[1] and outs[0].startswith(magic) and mod.decompress(outs[0]) == (tmp_path / "kept.paf").read_bytes()
