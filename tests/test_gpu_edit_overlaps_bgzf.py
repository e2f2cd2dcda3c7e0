"""filter / extract on BGZF overlap files as they are (yacrd_engine_edit_overlaps_bgzf_mem / _file: the compressed bytes go up,
the members are inflated in HBM while they land, the editor marks, scans and packs every text segment behind the launches
that decoded it) and on the text an ingest left in HBM (yacrd_engine_edit_overlaps_resident_mem / _file).  Every comparison
is exact.  The yardsticks, each pinned to the host loop and the reference's vectors by the existing suite: the ten-line
restatement, Engine.edit_overlaps_text, Engine.edit_overlaps_gzip and Engine.gzip."""
import bz2
import gzip
import os
import shutil
import struct
import subprocess
import threading

import numpy as np
import pytest

import inflate_cases as ic
import yacrd_amd
from deflate_cases import EOF_MEMBER
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, fuzz_cases, restate
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
TILE = 32768         # csrc/gpu_text.h: kGpTile
SEGMENT = 128 << 20  # csrc/gpu_text.h: kTextChunk * kTextSeg
BLOCK = 65280
OPS = (OP_FILTER, OP_EXTRACT)
CHUNKS = (7, 32769, 65280)

# the reference's unit vectors (src/editor/filter.rs:289-359, extract.rs:293-362) and their three reads, read 1 bad
_PAF_UNIT = (b"1\t12000\t20\t4500\t-\t2\t10000\t5500\t10000\t4500\t4500\t255\n"
             b"1\t12000\t5500\t10000\t-\t3\t10000\t0\t4500\t4500\t4500\t255\n"
             b"2\t1000\t0\t500\t+\t3\t1000\t500\t1000\t500\t500\t255\n")
_M4_UNIT = b"1 2 0.1 2 0 100 450 1000 0 550 900 1000\n1 3 0.1 2 0 550 900 1000 0 100 450 1000\n2 3 0.1 2 0 0 500 1000 0 500 1000 1000\n"
_UNIT_NAMES, _UNIT_TYPES = [b"1", b"2", b"3"], [yacrd_amd.NOT_COVERED, yacrd_amd.NOT_BAD, yacrd_amd.NOT_BAD]


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


def paf_to_m4(text):
    out = []
    for l in text.decode().split("\n"):
        f = l.split("\t")
        out.append(" ".join([f[0], f[5], "0.1", "2", "0", f[2], f[3], f[1], "1", f[7], f[8], f[6]]) if l else l)
    return "\n".join(out).encode()


def n_members(blob):
    """members of a stream built here (the BC subfield first in the extra field)"""
    n = at = 0
    while at < len(blob):
        assert blob[at + 12:at + 14] == b"BC"
        at += struct.unpack_from("<H", blob, at + 16)[0] + 1
        n += 1
    assert at == len(blob)
    return n


@pytest.fixture(scope="module")
def fixture_sets(engine, golden_dir):
    """[(name, text, fmt, names, types)]: the golden reads.paf under two detections, and its M4 rewrite"""
    paf = os.path.join(golden_dir, "reads.paf")
    text = open(paf, "rb").read()
    out = []
    for cov, ncov in ((0, 0.8), (4, 0.4)):
        res, names, _, _ = engine.ingest_paf(paf, cov, ncov)
        names = [n.encode() for n in names]
        out.append(("fixture %d %.1f" % (cov, ncov), text, 1, names, res.read_type.tolist()))
    out.append(("fixture as M4", paf_to_m4(text), 2, out[-1][3], out[-1][4]))
    return out


class Want:
    """what the yardsticks make of a text, once per (text, op): the kept bytes and the stream of them"""

    def __init__(self, engine, text, fmt, names, types):
        self.by_op = {}
        for op in OPS:
            kept, n_lines, n_kept = restate(text, op, dict(zip(names, types)), fmt == 2)
            assert kept == engine.edit_overlaps_text(op, text, names, types, fmt)
            stream = engine.edit_overlaps_gzip(op, text, names, types, fmt)
            assert stream == engine.gzip(kept)
            self.by_op[op] = (kept, stream, n_lines, n_kept)


def check(engine, blob, text, fmt, names, types, want, ctx):
    """both ops, both gzip_out, the stats"""
    for op in OPS:
        kept, stream, n_lines, n_kept = want.by_op[op]
        for gz in (False, True):
            got = engine.edit_overlaps_bgzf(op, blob, names, types, fmt, gzip_out=gz)  # (raises on YACRD_EFALLBACK)
            assert got == (stream if gz else kept), (ctx, op, gz)
            es, gs, us = engine.edit_stats, engine.gzip_stats, engine.inflate_stats
            assert (es["n_lines"], es["n_kept"], es["kept_bytes"], es["text_bytes"]) == (n_lines, n_kept, len(kept), len(text)), (ctx, op, gz)
            assert es["mirror_reused"] == 0
            assert us["n_members"] == n_members(blob) and us["in_bytes"] == len(blob) and us["out_bytes"] == len(text) and us["d2h_ms"] == 0, ctx
            assert (gs["in_bytes"], gs["out_bytes"]) == ((len(kept), len(stream)) if gz else (0, 0)), (ctx, op, gz)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,text", [(1, _PAF_UNIT), (2, _M4_UNIT)], ids=["paf", "m4"])
def test_reference_unit_vectors(engine, fmt, text):
    want = Want(engine, text, fmt, _UNIT_NAMES, _UNIT_TYPES)
    assert want.by_op[OP_FILTER][0] == text.split(b"\n")[2] + b"\n"  # (the two vector lines name read 1; the third does not)
    for chunk in CHUNKS:
        check(engine, ic.bgzf_of(text, chunk), text, fmt, _UNIT_NAMES, _UNIT_TYPES, want, chunk)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["0-0.8", "4-0.4", "m4"])
def test_fixture(engine, fixture_sets, tmp_path, which):
    name, text, fmt, names, types = fixture_sets[which]
    want = Want(engine, text, fmt, names, types)
    assert all(0 < len(want.by_op[op][0]) < len(text) for op in OPS)
    for chunk in CHUNKS:
        check(engine, ic.bgzf_of(text, chunk), text, fmt, names, types, want, (name, chunk))
    # the file form: the same bytes at out_path, nothing beside it
    blob = ic.bgzf_of(text)
    for op in OPS:
        for gz in (False, True):
            d = tmp_path / ("o%d%d" % (op, gz))
            d.mkdir()
            es, gs = engine.edit_overlaps_bgzf(op, blob, names, types, fmt, out_path=str(d / "k"), gzip_out=gz)
            assert os.listdir(d) == ["k"] and (d / "k").read_bytes() == want.by_op[op][1 if gz else 0]
            assert es["kept_bytes"] == len(want.by_op[op][0])


def test_fuzz_zero_fallbacks(engine):
    """every text of the fuzz set is taken (no NeedsHostParser), one chunk per case, rotating"""
    n = 0
    for tag, text, m4, names, types in fuzz_cases():
        fmt = 2 if m4 else 1
        chunk = CHUNKS[n % 3]
        blob = ic.bgzf_of(text, chunk, level=1)
        table = dict(zip(names, types))
        for op in OPS:
            kept, n_lines, n_kept = restate(text, op, table, m4)
            gz = bool((n + op) & 1)
            got = engine.edit_overlaps_bgzf(op, blob, names, types, fmt, gzip_out=gz)
            if gz:
                assert gzip.decompress(got) == kept and got == engine.gzip(kept), (tag, m4, op)
            else:
                assert got == kept, (tag, m4, op)
            es = engine.edit_stats
            assert (es["n_lines"], es["n_kept"], es["kept_bytes"], es["text_bytes"]) == (n_lines, n_kept, len(kept), len(text)), (tag, m4, op)
            assert engine.inflate_stats["d2h_ms"] == 0
        n += 1
    assert n >= 1000


# ---- 2. member borders where they hurt ----------------------------------------------------------------------------------------
def cut_at(text, cuts, level=6, eof_at=()):
    """`text` as BGZF with member borders exactly at `cuts` (and wherever a member would pass 65 280 bytes); an EOF member at `eof_at`"""
    out, at = [], 0
    for c in sorted(set(cuts)) + [len(text)]:
        while at < c:
            end = min(c, at + BLOCK)
            out.append(ic.member(text[at:end], level))
            at = end
        if c in eof_at:
            out.append(EOF_MEMBER)
    return b"".join(out) + EOF_MEMBER


@pytest.mark.parametrize("which", [1, 2], ids=["paf", "m4"])
def test_member_borders_where_they_hurt(engine, fixture_sets, which):
    _, full, fmt, names, types = fixture_sets[which]
    delim, ib = (b" ", 1) if fmt == 2 else (b"\t", 5)
    text = full[:full.index(b"\n", TILE + 4000) + 1]  # a few KiB beyond one tile
    want = Want(engine, text, fmt, names, types)
    line0 = text.index(b"\n", 2000) + 1
    nl = text.index(b"\n", line0)
    f = text[line0:nl].split(delim)
    second = line0 + sum(len(x) + 1 for x in f[:ib])
    assert len(f[0]) >= 2 and len(f[ib]) >= 2 and text[second:second + len(f[ib])] == f[ib]
    borders = {
        "between a newline and the next line": [nl + 1],
        "inside the first id": [line0 + 1],
        "inside the second id": [second + 1],
        "a one-byte member that is the newline": [nl, nl + 1],
        "tile border - 1": [TILE - 1],
        "tile border": [TILE],
        "tile border + 1": [TILE + 1],
        "every border at once": [line0 + 1, second + 1, nl, nl + 1, TILE - 1, TILE, TILE + 1],
    }
    for what, cuts in borders.items():
        check(engine, cut_at(text, cuts), text, fmt, names, types, want, what)
    check(engine, cut_at(text, [nl + 1, TILE], eof_at=[nl + 1]), text, fmt, names, types, want, "an EOF member in the middle")
    small = text[:text.index(b"\n", 400) + 1]
    assert 300 < len(small) < 1000
    check(engine, ic.bgzf_of(small, 1), small, fmt, names, types, Want(engine, small, fmt, names, types), "one-byte members throughout")


# ---- 3. the last line without its newline -------------------------------------------------------------------------------------
def test_the_last_line_without_its_newline(engine, fixture_sets):
    _, full, fmt, names, types = fixture_sets[1]
    text = full.rstrip(b"\n")
    want = Want(engine, text, fmt, names, types)
    with_nl = Want(engine, text + b"\n", fmt, names, types)
    assert all(want.by_op[op][:2] == with_nl.by_op[op][:2] for op in OPS)  # (the plain form adds the newline)
    for chunk in (100, BLOCK):
        check(engine, ic.bgzf_of(text, chunk), text, fmt, names, types, want, chunk)
    check(engine, cut_at(text, [len(text) - 1]), text, fmt, names, types, want, "the last member is one byte")


# ---- 4. across the mover's segment --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_text():
    """~132 MiB of PAF: short records over 3 000 reads (tests/test_gpu_ingest_bgzf.py's recipe)"""
    rng = np.random.default_rng(78)
    ids = ["r%05d" % i for i in range(3000)]
    block = []
    for k in range(20000):
        a, b = int(rng.integers(0, 3000)), int(rng.integers(0, 3000))
        s1, s2 = int(rng.integers(0, 8000)), int(rng.integers(0, 8000))
        block.append("%s\t9000\t%d\t%d\t-\t%s\t9000\t%d\t%d\n" % (ids[a], s1, s1 + int(rng.integers(1, 900)), ids[b], s2, s2 + int(rng.integers(1, 900))))
    unit = "".join(block).encode()
    text = unit * ((132 << 20) // len(unit) + 1)
    assert len(text) > SEGMENT + (4 << 20)
    return text


_BIG_NAMES = [b"r%05d" % i for i in range(3000)]
_BIG_TYPES = [1 if i % 7 == 0 else 2 if i % 11 == 0 else 0 for i in range(3000)]


@pytest.fixture(scope="module")
def big_want(big_text):
    with yacrd_amd.Engine(device_id=0) as e:
        return e.edit_overlaps_gzip(OP_FILTER, big_text, _BIG_NAMES, _BIG_TYPES, 1)


@pytest.mark.parametrize("stored", [True, False], ids=["stored", "level 1"])
def test_across_the_movers_segment(engine, big_text, big_want, stored):
    """stored members: the COMPRESSED stream crosses the 128 MiB segment; level 1: only the text does"""
    try:
        blob = ic.bgzf_of(big_text, stored=stored, level=1)
        assert len(blob) > SEGMENT + (4 << 20) if stored else len(blob) < SEGMENT
        assert engine.edit_overlaps_bgzf(OP_FILTER, blob, _BIG_NAMES, _BIG_TYPES, 1, gzip_out=True) == big_want
        assert engine.edit_stats["text_bytes"] == len(big_text) and 0 < engine.edit_stats["n_kept"] < engine.edit_stats["n_lines"]
    finally:
        engine.trim()


# ---- 5. refusals leave nothing behind -----------------------------------------------------------------------------------------
def refused(engine, tmp_path, blob, fmt=1, names=(b"a", b"b"), types=(0, 1)):
    """both forms refuse, nothing is left in the directory -> the message"""
    d = tmp_path / "refused"
    d.mkdir(exist_ok=True)
    msg = None
    for gz in (True, False):
        with pytest.raises(yacrd_amd.NeedsHostParser) as x:
            engine.edit_overlaps_bgzf(OP_EXTRACT, blob, list(names), list(types), fmt, gzip_out=gz)
        msg = str(x.value)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps_bgzf(OP_EXTRACT, blob, list(names), list(types), fmt, out_path=str(d / "out.paf.gz"), gzip_out=gz)
        assert os.listdir(d) == [], "no file and no temporary beside out_path"
    return msg


_GOOD = b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\t255\n"


def usable(engine):
    assert engine.edit_overlaps_bgzf(OP_EXTRACT, ic.bgzf_of(_GOOD * 5, 7), [b"a", b"b"], [0, 1], 1) == engine.gzip(_GOOD * 5)


def test_what_is_not_bgzf(engine, tmp_path):
    text = _GOOD * 50
    assert "not BGZF" in refused(engine, tmp_path, gzip.compress(text, 1))
    assert "not BGZF" in refused(engine, tmp_path, bz2.compress(text))
    for name, blob in ic.not_bgzf_cases():
        assert "not BGZF" in refused(engine, tmp_path, blob), name
    usable(engine)


def test_a_member_the_decoder_does_not_take(engine, tmp_path):
    """one damaged member per cause the decoder names, behind good members: the status word wins over what the kernels made of the text"""
    good = ic.bgzf_of(_GOOD * 3000, 40000)[:-len(EOF_MEMBER)]
    assert n_members(good) >= 2
    seen = set()
    for name, blob, cause in ic.not_taken_cases():
        if cause in seen or name == "a refused member behind good ones":
            continue
        seen.add(cause)
        bad = blob[:-len(EOF_MEMBER)]
        msg = refused(engine, tmp_path, good + bad + good + EOF_MEMBER)
        assert cause in msg and "does not take" in msg, (name, msg)
    assert len(seen) == 12
    usable(engine)


def test_the_plain_forms_own_causes_inside_valid_bgzf(engine, tmp_path):
    odd = [b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\t\"x\"\n", b"a\t10\t0\t5\t+\tb\t10\t0\r5\t5\t5\t255\n", b"a\t10\t0\t5\t+\tb\t10\t0\t5\t5\t5\n"]
    for line in odd:
        text = _GOOD * 3 + line + _GOOD * 2
        with pytest.raises(yacrd_amd.NeedsHostParser) as plain:
            engine.edit_overlaps_text(OP_EXTRACT, text, [b"a", b"b"], [0, 1], 1)
        for chunk in (7, BLOCK):
            assert refused(engine, tmp_path, ic.bgzf_of(text, chunk)) == str(plain.value)
    usable(engine)


def test_a_damaged_member_behind_the_first_text_segment(engine, tmp_path, big_text):
    """more than 128 MiB of good text, every member whole lines, then a member whose CRC does not match: the first segment is
    valid, so what it keeps has been written beside out_path by the time the status word refuses; still nothing is left there"""
    try:
        unit = big_text[:big_text.rindex(b"\n", 0, BLOCK) + 1]  # whole lines, as many as a member holds
        assert unit.endswith(b"\n") and BLOCK - 200 < len(unit) <= BLOCK
        n = (SEGMENT + (4 << 20)) // len(unit) + 40  # (the damaged member lies behind the first segment and the chunk its marks may read)
        m = ic.member(unit, 1)
        bad = bytearray(m)
        bad[-8] ^= 1  # (the CRC-32 field: the member's text is what it was, only the decoder refuses it)
        good = m * n + EOF_MEMBER
        blob = m * (n - 3) + bytes(bad) + m * 3 + EOF_MEMBER
        assert (n - 3) * len(unit) > SEGMENT + (4 << 20)
        d = tmp_path / "big"
        d.mkdir()
        # the same stream without the damage is taken, and keeps bytes in its first segment: the yardstick for "valid"
        es, _ = engine.edit_overlaps_bgzf(OP_EXTRACT, good, _BIG_NAMES, _BIG_TYPES, 1, out_path=str(d / "good.paf"), gzip_out=False)
        kept_unit = restate(unit, OP_EXTRACT, dict(zip(_BIG_NAMES, _BIG_TYPES)), False)[0]
        assert len(kept_unit) > 1000 and es["kept_bytes"] == n * len(kept_unit) == os.path.getsize(d / "good.paf")
        os.remove(d / "good.paf")
        for gz in (False, True):
            # what lies beside out_path while the call runs: the largest file seen (the call releases the interpreter lock)
            seen, stop = [0], threading.Event()

            def watch():
                while not stop.is_set():
                    for name in os.listdir(d):
                        try:
                            seen[0] = max(seen[0], os.path.getsize(d / name))
                        except OSError:
                            pass

            t = threading.Thread(target=watch)
            t.start()
            try:
                with pytest.raises(yacrd_amd.NeedsHostParser) as x:
                    engine.edit_overlaps_bgzf(OP_EXTRACT, blob, _BIG_NAMES, _BIG_TYPES, 1, out_path=str(d / "out.paf.gz"), gzip_out=gz)
            finally:
                stop.set()
                t.join()
            assert "CRC" in str(x.value) and "does not take" in str(x.value)
            assert seen[0] > 0, "the sink had been written to when the status word refused"
            assert os.listdir(d) == []
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps_bgzf(OP_EXTRACT, blob, _BIG_NAMES, _BIG_TYPES, 1)
        usable(engine)
    finally:
        engine.trim()


# ---- 6. resident --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [1, 2], ids=["paf", "m4"])
def test_resident(engine, fixture_sets, golden_dir, tmp_path, which):
    _, text, fmt, names, types = fixture_sets[which]
    want = Want(engine, text, fmt, names, types)

    def both(ctx):
        for op in OPS:
            kept, stream, n_lines, n_kept = want.by_op[op]
            assert engine.edit_overlaps_resident(op, names, types) == stream, (ctx, op)
            es, gs = engine.edit_stats, engine.gzip_stats
            assert es["mirror_reused"] == 1 and es["text_ms"] == 0 and es["text_bytes"] == len(text), ctx
            assert (es["n_lines"], es["n_kept"], es["kept_bytes"]) == (n_lines, n_kept, len(kept)) and gs["in_bytes"] == len(kept), ctx
            assert engine.edit_overlaps_resident(op, names, types, gzip_out=False) == kept, (ctx, op)
            assert engine.gzip_stats["in_bytes"] == 0
            out = tmp_path / "res.gz"
            engine.edit_overlaps_resident(op, names, types, out_path=str(out))
            assert out.read_bytes() == stream
            out.unlink()

    for chunk in (7, BLOCK):
        engine.ingest_bgzf(ic.bgzf_of(text, chunk), 4, 0.4, fmt=fmt)
        both("ingest_bgzf %d" % chunk)
    engine.report_text()  # (the CLI's order: the report writer runs between the ingest and the edit)
    both("behind the report writer")
    engine.ingest_text(text, 4, 0.4, fmt=fmt)
    both("ingest_text")
    open_end = text.rstrip(b"\n")
    engine.ingest_bgzf(ic.bgzf_of(open_end, 100), 4, 0.4, fmt=fmt)  # (the added newline: the plain form's bytes)
    assert engine.edit_overlaps_resident(OP_FILTER, names, types, gzip_out=False) == want.by_op[OP_FILTER][0]
    if fmt == 1:
        paf = tmp_path / "reads.paf"
        shutil.copy(os.path.join(golden_dir, "reads.paf"), paf)
        engine.ingest_paf(str(paf), 4, 0.4)
        both("ingest_paf")


def test_no_resident_text_is_the_callers_error(fixture_sets, golden_dir):
    _, text, fmt, names, types = fixture_sets[1]

    def no_text(e):
        with pytest.raises(yacrd_amd.EngineError, match="no overlap text is resident") as x:
            e.edit_overlaps_resident(OP_FILTER, names, types)
        assert not isinstance(x.value, yacrd_amd.NeedsHostParser)

    with yacrd_amd.Engine(device_id=0) as e:
        no_text(e)  # a fresh engine
        e.ingest_bgzf(ic.bgzf_of(text), 4, 0.4)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            e.ingest_bgzf(gzip.compress(text, 1), 4, 0.4)
        no_text(e)  # after a refused ingest
        e.ingest_bgzf(ic.bgzf_of(text), 4, 0.4)
        e.trim()
        no_text(e)
        e.ingest_bgzf(ic.bgzf_of(text), 4, 0.4)
        e.ingest_report(os.path.join(golden_dir, "truth.yacrd"), 0.4)
        no_text(e)


def test_a_file_never_takes_an_anonymous_mirror(engine, fixture_sets, tmp_path):
    """edit_overlaps(path) after ingest_text / ingest_bgzf of the same bytes: equal size, no identity -> the text is moved"""
    _, text, fmt, names, types = fixture_sets[1]
    paf = tmp_path / "x.paf"
    paf.write_bytes(text)
    want = restate(text, OP_FILTER, dict(zip(names, types)), False)[0]
    for ingest in (lambda: engine.ingest_text(text, 4, 0.4), lambda: engine.ingest_bgzf(ic.bgzf_of(text), 4, 0.4)):
        ingest()
        st = engine.edit_overlaps(OP_FILTER, str(paf), str(tmp_path / "y.paf"), names, types)
        assert st["mirror_reused"] == 0 and (tmp_path / "y.paf").read_bytes() == want


# ---- 7. buffers ---------------------------------------------------------------------------------------------------------------
def test_buffers_go_with_trim_and_the_engine(fixture_sets):
    _, text, fmt, names, types = fixture_sets[1]
    before = live_bytes()
    blob = ic.bgzf_of(text, level=1)
    with yacrd_amd.Engine(device_id=0) as e:
        e.edit_overlaps_bgzf(OP_FILTER, blob, names, types, fmt)
        e.ingest_bgzf(blob, 4, 0.4)
        e.trim()
        # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers, the batch path's buffers
        # the ingest ran its sweep in)
        warm = live_bytes()
        e.edit_overlaps_bgzf(OP_FILTER, blob, names, types, fmt)
        e.ingest_bgzf(blob, 4, 0.4)
        e.edit_overlaps_resident(OP_EXTRACT, names, types)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            e.edit_overlaps_bgzf(OP_FILTER, blob[:-3], names, types, fmt)
        assert live_bytes()[0] > warm[0] + len(text) + len(blob)
        e.trim()
        assert live_bytes() == warm
    assert live_bytes() == before


# ---- 8. the CLI ---------------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    base = {k: v for k, v in os.environ.items() if k not in ("YACRD_DEVICE_INFLATE", "YACRD_NO_DEVICE_INFLATE")}
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(base, **env))


def _line(p):
    hit = [l for l in p.stdout.splitlines() if l.startswith("[info] device editor + deflate:")]
    assert len(hit) == 1, p.stdout + p.stderr
    return hit[0]


@pytest.fixture(scope="module")
def cli_work(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("edit_bgzf_cli")
    text = open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    blob = ic.bgzf_of(text, level=6)
    (d / "x.paf.gz").write_bytes(blob)
    (d / "copy.paf.gz").write_bytes(blob)
    (d / "plain.paf.gz").write_bytes(gzip.compress(text, 1))
    return d, text


@pytest.mark.parametrize("op", ["filter", "extract"])
def test_cli_routes(cli_work, op):
    d, text = cli_work
    det = ["-c", "4", "-n", "0.4"]
    x = d / "x.paf.gz"

    def run(tag, src, sub_in, *more, **env):
        out, rep = d / ("%s_%s.paf.gz" % (op, tag)), d / ("%s_%s.yacrd" % (op, tag))
        p = _cli(["-i", src, "-o", rep] + det + list(more) + [op, "-i", sub_in, "-o", out], YACRD_CLI_TIMING="1", **env)
        assert p.returncode == 0, p.stderr
        return p, out.read_bytes(), rep.read_bytes()

    # today's route, switched off outright: the yardstick
    p0, want, want_rep = run("off", x, x, YACRD_NO_DEVICE_INFLATE="1")
    assert "device_inflate=0" in _line(p0) and "resident=0" in _line(p0) and "text_reused=1" in _line(p0) and "[timing] inflate" in p0.stderr
    assert 0 < len(gzip.decompress(want)) < len(text)
    # the same BGZF file: ingested compressed, edited where the ingest left it
    p, got, rep = run("same", x, x, YACRD_DEVICE_INFLATE="1")
    assert "resident=1 device_inflate=1" in _line(p) and "text_reused=1" in _line(p)
    assert "[timing] inflate" not in p.stderr and "[info] device inflate:" in p.stderr
    assert got == want and rep == want_rep
    # another BGZF file (a copy, another inode): the editor's own _bgzf_ form
    p, got, rep = run("other", x, d / "copy.paf.gz", YACRD_DEVICE_INFLATE="1")
    assert "resident=0 device_inflate=1" in _line(p) and "text_reused=0" in _line(p)
    assert got == want and rep == want_rep
    # plain gzip, the same file: today's line
    plain = d / "plain.paf.gz"
    p, got, rep = run("plain", plain, plain, YACRD_DEVICE_INFLATE="1")
    assert "resident=0 device_inflate=0" in _line(p) and "text_reused=1" in _line(p) and "[timing] inflate" in p.stderr
    assert got == want and rep == want_rep
    # YACRD_NO_DEVICE_INFLATE=1 wins over YACRD_DEVICE_INFLATE=1; --gpus 2 never tries
    p, got, rep = run("both", x, x, YACRD_DEVICE_INFLATE="1", YACRD_NO_DEVICE_INFLATE="1")
    assert "resident=0 device_inflate=0" in _line(p) and got == want and rep == want_rep
    p, got, rep = run("gpus2", x, x, "--gpus", "2", YACRD_DEVICE_INFLATE="1", YACRD_GPUS_ON_DEVICE="0")
    assert "resident=0 device_inflate=0" in _line(p) and got == want and rep == want_rep
    assert not [n for n in os.listdir(d) if ".gz." in n], "no temporary is left"


@pytest.mark.parametrize("op", ["filter", "extract"])
def test_cli_a_quoted_field_inside_bgzf(golden_dir, tmp_path, op):
    """the host path's bytes, by the host path"""
    text = open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    lines = text.split(b"\n")
    lines[700] = lines[700] + b"\t\"cg:Z:5M\""
    quoted = b"\n".join(l if i == 700 or not l else l + b"\tcg:Z:5M" for i, l in enumerate(lines))
    x = tmp_path / "q.paf.gz"
    x.write_bytes(ic.bgzf_of(quoted))
    runs = []
    for env in ({"YACRD_NO_DEVICE_EDITOR": "1", "YACRD_NO_DEVICE_INFLATE": "1"}, {"YACRD_DEVICE_INFLATE": "1"}):
        o = tmp_path / ("q%d.paf.gz" % len(runs))
        p = _cli(["-i", x, "-o", tmp_path / ("q%d.yacrd" % len(runs))] + ["-c", "4", "-n", "0.4", op, "-i", x, "-o", o], YACRD_CLI_TIMING="1", **env)
        assert "[info] device editor" not in p.stderr + p.stdout
        runs.append((p.returncode, [l for l in p.stderr.splitlines() if l.startswith("Error")], o.read_bytes() if o.exists() else None))
    assert runs[0] == runs[1] and runs[0][0] == 0 and runs[0][2] is not None
    assert (tmp_path / "q0.yacrd").read_bytes() == (tmp_path / "q1.yacrd").read_bytes()
    assert not [n for n in os.listdir(tmp_path) if ".gz." in n], "no temporary is left"
