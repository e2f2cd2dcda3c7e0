"""yacrd_engine_ingest_overlaps_bgzf_mem / yacrd_engine_ingest_report_bgzf_mem — a BGZF overlap file or report ingested as it
is: the compressed bytes go up, the members are inflated in HBM while they land (csrc/bgzf_plan.h names what to launch), and
the device parser / report reader take the text from there.  Against the oracle on the host parser's CSR, bit for bit against
Engine.ingest_text / ingest_report of the plain text, over member borders placed where they hurt, across the mover's 128 MiB
segment in both streams, and through every refusal; then the CLI's routes."""
import bz2
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import inflate_cases as ic
import oracle
import report_cases as rc
import yacrd_amd
from cases import assert_same
from deflate_cases import EOF_MEMBER
from input_csr_cases import assert_same_csr
from yacrd_amd import host
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
TILE = 32768         # the parser's tile (csrc/gpu_text.h: kGpTile)
SEGMENT = 128 << 20  # what the mover hands on at once
BLOCK = 65280


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


def paf_to_m4(text):
    out = []
    for l in text.split("\n"):
        f = l.split("\t")
        out.append(" ".join([f[0], f[5], "0.1", "2", "0", f[2], f[3], f[1], "1", f[7], f[8], f[6]]) if l else l)
    return "\n".join(out)


@pytest.fixture(scope="module")
def texts(golden_dir, tmp_path_factory):
    """{name: (text bytes, fmt, coverage, not_coverage)}: the reference fixture, its M4 rewrite, a synthetic PAF"""
    with open(os.path.join(golden_dir, "reads.paf"), newline="") as f:
        fixture = f.read()
    p = str(tmp_path_factory.mktemp("bgzf_ingest") / "s.paf")
    host.synth_paf(host.SYNTH_ONT, 3000, 60000, 15, p)
    with open(p, "rb") as f:
        synth = f.read()
    return {"fixture": (fixture.encode(), 1, 0, 0.8), "fixture as M4": (paf_to_m4(fixture).encode(), 2, 0, 0.8), "synthetic": (synth, 1, 4, 0.4)}


@pytest.fixture(scope="module")
def wanted(texts):
    """per text, once: what the oracle makes of the oracle's parse -> (names, (off, iv, ln), (bad_offsets, bad_regions, read_type))"""
    out = {}
    for name, (text, fmt, cov, nc) in texts.items():
        reads = (oracle.parse_m4 if fmt == 2 else oracle.parse_paf)(text.decode())
        w_names, off, iv, ln = oracle.to_csr(reads)
        out[name] = (list(w_names), (off, iv, ln), oracle.run(off, iv, ln, cov, nc, n_threads=4))
    return out


def n_members(blob):
    """members of a stream built here (the BC subfield first in the extra field), without copying the stream"""
    n = at = 0
    while at < len(blob):
        assert blob[at + 12:at + 14] == b"BC"
        at += struct.unpack_from("<H", blob, at + 16)[0] + 1
        n += 1
    assert at == len(blob)
    return n


def same_as_plain(engine, blob, text, fmt, cov, nc, ctx):
    """ingest_bgzf(blob) equals ingest_text(text) bit for bit, and the device inflated every member of the walk"""
    plain, p_names, p_lengths, p_stats = engine.ingest_text(text, cov, nc, fmt=fmt)
    got, names, lengths, stats = engine.ingest_bgzf(blob, cov, nc, fmt=fmt)
    assert names == p_names and np.array_equal(lengths, p_lengths), ctx
    assert_same(got, (plain.bad_offsets, plain.bad_regions, plain.read_type), ctx)
    assert stats["n_reads"] == p_stats["n_reads"] and stats["n_records"] == p_stats["n_records"], ctx
    inf = stats["inflate"]
    assert stats["text_bytes"] == len(text) == inf["out_bytes"] and inf["in_bytes"] == len(blob), ctx
    assert inf["n_members"] == n_members(blob), ctx
    assert inf["d2h_ms"] == 0
    return got, names, lengths, stats


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [TILE, TILE + 1, BLOCK])
@pytest.mark.parametrize("name", ["fixture", "fixture as M4", "synthetic"])
def test_parity_with_the_oracle_and_the_plain_text(engine, texts, wanted, name, chunk):
    text, fmt, cov, nc = texts[name]
    w_names, csr, want = wanted[name]
    got, names, lengths, stats = same_as_plain(engine, ic.bgzf_of(text, chunk=chunk), text, fmt, cov, nc, (name, chunk))
    assert names == w_names and np.array_equal(lengths.astype(np.uint64), csr[2])
    assert stats["n_records"] * 2 == int(csr[0][-1])
    assert_same_csr(engine.debug_input_csr(), csr, name)  # the CSR the parse built in HBM, interval by interval
    assert_same(got, want, name)


@pytest.mark.parametrize("chunk", [1, 7, 100])
def test_members_of_a_few_bytes(engine, texts, chunk):
    """the smallest members, on a text of a few hundred bytes: every byte its own member, members that share dwords"""
    lines = texts["fixture"][0].split(b"\n")
    text = b"\n".join(lines[:6]) + b"\n"
    assert 200 < len(text) < 1000
    reads = oracle.parse_paf(text.decode())
    w_names, off, iv, ln = oracle.to_csr(reads)
    got, names, lengths, _ = same_as_plain(engine, ic.bgzf_of(text, chunk=chunk), text, 1, 0, 0.8, chunk)
    assert names == list(w_names)
    assert_same_csr(engine.debug_input_csr(), (off, iv, ln), "chunk %d" % chunk)
    assert_same(got, oracle.run(off, iv, ln, 0, 0.8, n_threads=2), "chunk %d" % chunk)


def cut_at(text, cuts, level=6):
    """`text` as BGZF with member borders exactly at `cuts` (and wherever a member would pass 65 280 bytes)"""
    out, at = [], 0
    for c in sorted(set(cuts)) + [len(text)]:
        while at < c:
            end = min(c, at + BLOCK)
            out.append(ic.member(text[at:end], level))
            at = end
    return b"".join(out) + EOF_MEMBER


def test_member_borders_where_they_hurt(engine, texts):
    text, fmt, cov, nc = texts["synthetic"]
    assert len(text) > 4 * TILE
    line0 = text.index(b"\n", 2 * TILE) + 1  # a line that begins behind the second tile boundary
    f = text[line0:text.index(b"\n", line0)].split(b"\t")
    number = line0 + len(f[0]) + 1 + len(f[1]) // 2 + 1  # inside the length column
    assert len(f[0]) >= 2 and len(f[1]) >= 3 and text[number - 1:number + 1].isdigit()
    nl = text.index(b"\n", line0)
    line_end = text.index(b"\n", nl + 1)
    borders = {
        "inside a read id": [line0 + 1],
        "inside a number": [number],
        "in front of the newline": [nl],
        "behind the newline": [nl + 1],
        "on a tile boundary": [TILE, 2 * TILE, 3 * TILE],
        "a line in three members": [nl + 1 + (line_end - nl) // 3, nl + 1 + 2 * (line_end - nl) // 3],
        "every border at once": [line0 + 1, number, nl, nl + 1, TILE, 2 * TILE, line_end - 1],
    }
    for what, cuts in borders.items():
        same_as_plain(engine, cut_at(text, cuts), text, fmt, cov, nc, what)


def outcome(call):
    try:
        got, names, lengths, _ = call()
    except yacrd_amd.NeedsHostParser:
        return "host parser"
    return names, lengths.tolist(), got.bad_offsets.tolist(), got.bad_regions.tolist(), got.read_type.tolist()


def test_a_last_member_that_ends_without_a_newline(engine, texts):
    """whatever ingest_text makes of a text whose last line has no newline — its result, or a refusal — ingest_bgzf makes too"""
    text = texts["fixture"][0].rstrip(b"\n")
    assert not text.endswith(b"\n")
    for chunk in (100, BLOCK):
        blob = ic.bgzf_of(text, chunk=chunk)
        assert outcome(lambda: engine.ingest_bgzf(blob, 0, 0.8)) == outcome(lambda: engine.ingest_text(text, 0, 0.8))


# ---- the mover's segment border -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_text():
    """~132 MiB of PAF: short records over 3 000 reads"""
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


@pytest.mark.parametrize("stored", [True, False], ids=["stored", "level 1"])
def test_across_the_movers_segment(engine, big_text, stored):
    """stored members: the COMPRESSED stream crosses the 128 MiB segment, members are launched in two steps and lie across the
    border; level 1: the compressed stream is under one segment and the TEXT over one, handed on in two.  Against ingest_text,
    which the existing suite pins to the oracle at this size."""
    try:
        blob = ic.bgzf_of(big_text, stored=stored, level=1)
        assert (len(blob) > SEGMENT + (4 << 20) and SEGMENT % (BLOCK + 31) != 0) if stored else len(blob) < SEGMENT
        same_as_plain(engine, blob, big_text, 1, 3, 0.4, "stored" if stored else "level 1")
    finally:
        engine.trim()


def test_the_second_parse_from_hbm(engine):
    """The room for the records comes from the line density of the first members' text (at most 1 MiB of it, decoded on the
    host, + 25 % + 4096): a text that opens with long lines and goes on with short ones outgrows it, and the parse is repeated
    with the exact number over the text that lies inflated in HBM."""
    rng = np.random.default_rng(79)
    ids = ["r%05d" % i for i in range(3000)]
    pad = "x" * 2000
    head = "".join("%s\t9000\t%d\t%d\t+\t%s\t9000\t%d\t%d\ttg:Z:%s\n" % (ids[k % 50], k, k + 500, ids[(k * 7 + 1) % 50], 2 * k, 2 * k + 700, pad)
                   for k in range(700))
    tail = "".join("%s\t9000\t%d\t%d\t-\t%s\t9000\t%d\t%d\n" % (ids[int(rng.integers(0, 3000))], s, s + 100, ids[int(rng.integers(0, 3000))], s + 7, s + 300)
                   for s in range(80000))
    text = (head + tail).encode()
    blob = ic.bgzf_of(text, level=1)
    sampled = ((1 << 20) // BLOCK) * BLOCK  # the members that fit 1 MiB
    estimate = int(len(text) / sampled * text[:sampled].count(b"\n") * 1.25) + 4096
    assert len(head) > sampled and estimate < 700 + 80000 < len(text) // 17  # the estimate falls short, the bound would not
    got, names, lengths, stats = same_as_plain(engine, blob, text, 1, 3, 0.4, "skewed line lengths")
    assert stats["n_records"] == 700 + 80000
    c = host.csr_from_memory(text, host.FMT_PAF, n_threads=4)
    assert names == c.names and np.array_equal(lengths, c.lengths)
    assert_same(got, oracle.run(c.offsets, c.intervals, c.lengths.astype(np.uint64), 3, 0.4, n_threads=4), "skewed line lengths")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refused(engine, blob, fmt=1):
    with pytest.raises(yacrd_amd.NeedsHostParser) as x:
        engine.ingest_bgzf(blob, 0, 0.8, fmt=fmt)
    return str(x.value)


def test_refusals_leave_the_engine_usable(engine, texts, wanted):
    text = texts["fixture"][0]
    good = ic.bgzf_of(text, chunk=40000)[:-len(EOF_MEMBER)]
    assert n_members(good) >= 2
    assert "not BGZF" in refused(engine, gzip.compress(text, 1))
    assert "not BGZF" in refused(engine, bz2.compress(text))
    cases = ic.not_bgzf_cases()
    assert len(cases) == 13
    for name, blob in cases:
        assert "not BGZF" in refused(engine, blob), name
    # one member per cause the decoder names, behind members that are taken
    seen = set()
    for name, blob, cause in ic.not_taken_cases():
        if cause in seen or name == "a refused member behind good ones":
            continue
        seen.add(cause)
        assert blob.endswith(EOF_MEMBER) and len(ic.walk(blob)) == 2
        bad = blob[:-len(EOF_MEMBER)]
        msg = refused(engine, good + bad + EOF_MEMBER)
        assert cause in msg and "does not take" in msg, (name, msg)
    assert len(seen) == 12
    # the parser's own causes, inside valid BGZF
    row = b"a\t100\t1\t50\t+\tb\t200\t2\t60\n"
    for bad_text in (b'"a"\t100\t1\t50\t+\tb\t200\t2\t60\n', b"a\t100\t1\t50\t+\tb\t200\t2\t60\t1\rb\t9\t0\t1\t+\ta\t100\t5\t6\n",
                     b"a\t0x64\t1\t50\t+\tb\t200\t2\t60\n"):
        for chunk in (7, BLOCK):
            assert "host parser" in refused(engine, ic.bgzf_of(row * 3 + bad_text + row, chunk=chunk))
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.ingest_text(row * 3 + bad_text + row, 0, 0.8)
    # nothing is left behind: no resident table, no input CSR; and the engine ingests the fixture as before
    assert engine.debug_input_csr() is None
    with pytest.raises(yacrd_amd.EngineError):
        engine.report_text()
    w_names, _, want = wanted["fixture"]
    got, names, _, _ = engine.ingest_bgzf(ic.bgzf_of(text), 0, 0.8)
    assert names == w_names
    assert_same(got, want, "after the refusals")


def test_a_damaged_member_behind_the_first_text_segment(engine, big_text):
    """more than 128 MiB of good text — the parser has run over the first segment — then a member whose CRC does not match"""
    try:
        n = SEGMENT // BLOCK + 40
        m = ic.member(big_text[:BLOCK], 1)
        bad = bytearray(m)
        bad[-8] ^= 1
        msg = refused(engine, m * (n - 3) + bytes(bad) + m * 3 + EOF_MEMBER)
        assert "CRC" in msg and "does not take" in msg
        assert engine.debug_input_csr() is None
    finally:
        engine.trim()


def test_buffers_go_with_trim_and_the_engine(texts):
    before = live_bytes()
    text = texts["synthetic"][0]
    blob = ic.bgzf_of(text, level=1)
    with yacrd_amd.Engine(device_id=0) as e:
        e.ingest_bgzf(blob, 4, 0.4)
        e.trim()
        warm = live_bytes()  # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers)
        e.ingest_bgzf(blob, 4, 0.4)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            e.ingest_bgzf(blob[:-3], 4, 0.4)
        held = live_bytes()
        assert held[0] > warm[0] + len(text) + len(blob)
        e.trim()
        assert live_bytes() == warm
    assert live_bytes() == before


# ---- reports ------------------------------------------------------------------------------------------------------------------
def report_texts():
    rows = [b"NotBad\tr%d\t%d\t1,0,%d\n" % (i, 1000 + i, i + 1) for i in range(6000)]
    rows[0] = b"Chimeric\tdup\t11\t1,2,3;4,5,6\n"
    rows[4999] = b"NotBad\tdup\t22\t\n"
    rows[-1] = b"NotCovered\tdup\t33\t7,8,9"  # the last line, without a newline
    return {"duplicate ids, the last row wins": b"".join(rows),
            "empty regions": b"NotBad\ta\t10\t\nNotCovered\tb\t20\t20,0,20\nNotBad\tc\t30\t\n",
            "fuzz text": rc.make_text(7, 200000),
            "no lines": b"\n\r\n\n"}


def report_outcome(call):
    try:
        res, names, lengths, stats = call()
    except yacrd_amd.NeedsHostParser:
        return "host reader"
    return names, lengths.tolist(), res.bad_offsets.tolist(), res.bad_regions.tolist(), res.read_type.tolist(), stats["n_records"]


@pytest.mark.parametrize("chunk", [1, 100, BLOCK])
def test_reports_equal_the_plain_reader(engine, chunk):
    for name, text in report_texts().items():
        if chunk == 1 and len(text) > 2000:
            text = text[:text.index(b"\n", 1500) + 1]  # (a member per byte: a few hundred members)
        blob = ic.bgzf_of(text, chunk=chunk)
        want = report_outcome(lambda: engine.ingest_report(text, 0.4))
        assert want != "host reader", name
        res, names, lengths, stats = engine.ingest_report_bgzf(blob, 0.4)
        assert (names, lengths.tolist(), res.bad_offsets.tolist(), res.bad_regions.tolist(), res.read_type.tolist(), stats["n_records"]) == want, name
        assert stats["text_bytes"] == len(text) and stats["inflate"]["n_members"] == n_members(blob), name


def test_report_refusals(engine):
    good = ic.member(rc.GOOD_ROW * 50)
    for name in rc.CORRUPT:
        text = rc.corrupt_text(name)
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.ingest_report(text, 0.4)
        for chunk in (7, BLOCK):
            with pytest.raises(yacrd_amd.NeedsHostParser) as x:
                engine.ingest_report_bgzf(ic.bgzf_of(text, chunk=chunk), 0.4)
            assert "host reader" in str(x.value), name
    for blob in (gzip.compress(rc.GOOD_ROW, 1), bz2.compress(rc.GOOD_ROW)):
        with pytest.raises(yacrd_amd.NeedsHostParser) as x:
            engine.ingest_report_bgzf(blob, 0.4)
        assert "not BGZF" in str(x.value)
    bad = bytearray(good)
    bad[-8] ^= 1
    with pytest.raises(yacrd_amd.NeedsHostParser) as x:
        engine.ingest_report_bgzf(good + bytes(bad) + EOF_MEMBER, 0.4)
    assert "CRC" in str(x.value)
    # an empty member that is not taken, in a stream of no text
    with pytest.raises(yacrd_amd.NeedsHostParser) as x:
        engine.ingest_report_bgzf(ic.frame(b"", b"") + EOF_MEMBER, 0.4)
    assert "ends early" in str(x.value)
    res, names, _, _ = engine.ingest_report_bgzf(good + EOF_MEMBER, 0.4)
    assert names == ["read-ok"]


# ---- the resident table ---------------------------------------------------------------------------------------------------------
def test_the_resident_table_writes_the_same_report(engine, texts):
    text, fmt, cov, nc = texts["synthetic"]
    engine.ingest_text(text, cov, nc, fmt=fmt)
    want = engine.report_text()
    engine.ingest_bgzf(ic.bgzf_of(text, chunk=TILE + 1), cov, nc, fmt=fmt)
    assert engine.report_text() == want and want.count(b"\n") == 3000


# ---- the CLI ------------------------------------------------------------------------------------------------------------------
def cli(args, **env):
    e = dict(os.environ, YACRD_CLI_TIMING="1")
    e.pop("YACRD_NO_DEVICE_INFLATE", None)
    e.pop("YACRD_DEVICE_INFLATE", None)
    e.update(env)
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def stderr_lines(p, head):
    return [l for l in p.stderr.splitlines() if l.startswith(head)]


@pytest.fixture(scope="module")
def cli_work(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_cli")
    paf = open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    (d / "bgzf.paf.gz").write_bytes(ic.bgzf_of(paf, chunk=50000))
    (d / "plain.paf.gz").write_bytes(gzip.compress(paf, 1))
    rep = open(os.path.join(golden_dir, "truth.yacrd"), "rb").read()
    (d / "bgzf.yacrd.gz").write_bytes(ic.bgzf_of(rep, chunk=3000))
    with open(os.path.join(golden_dir, "truth.yacrd")) as f:
        truth = set(l.rstrip("\n") for l in f)
    return d, truth, len(paf), len(rep)


def report_set(path):
    with open(path) as f:
        return set(l.rstrip("\n") for l in f)


def test_cli_bgzf_overlaps_take_the_device_inflate(cli_work):
    """(an overlap file takes the route with YACRD_DEVICE_INFLATE=1: DESIGN 7i's measurement left it opt-in; a report by default)"""
    d, truth, n_paf, _ = cli_work
    p = cli(["-i", d / "bgzf.paf.gz", "-o", d / "a.yacrd"], YACRD_DEVICE_INFLATE="1")
    assert report_set(d / "a.yacrd") == truth
    inf = stderr_lines(p, "[info] device inflate:")
    assert len(inf) == 1 and (" %d -> %d bytes" % (os.path.getsize(d / "bgzf.paf.gz"), n_paf)) in inf[0], p.stderr
    assert "[timing] inflate" not in p.stderr and len(stderr_lines(p, "[info] device parser:")) == 1


def test_cli_plain_gzip_takes_the_host_inflate(cli_work):
    d, truth, _, _ = cli_work
    p = cli(["-i", d / "plain.paf.gz", "-o", d / "b.yacrd"], YACRD_DEVICE_INFLATE="1")
    assert report_set(d / "b.yacrd") == truth
    assert "[timing] inflate" in p.stderr and not stderr_lines(p, "[info] device inflate:") and len(stderr_lines(p, "[info] device parser:")) == 1


def test_cli_switch_and_several_engines_take_the_old_route(cli_work):
    d, truth, _, _ = cli_work
    p = cli(["-i", d / "bgzf.paf.gz", "-o", d / "c.yacrd"], YACRD_DEVICE_INFLATE="1", YACRD_NO_DEVICE_INFLATE="1")
    assert report_set(d / "c.yacrd") == truth
    assert "[timing] inflate" in p.stderr and not stderr_lines(p, "[info] device inflate:")
    p = cli(["-i", d / "bgzf.paf.gz", "-o", d / "e.yacrd", "--gpus", "2"], YACRD_DEVICE_INFLATE="1", YACRD_GPUS_ON_DEVICE="0")
    assert report_set(d / "e.yacrd") == truth
    assert "[timing] inflate" in p.stderr and not stderr_lines(p, "[info] device inflate:")


def test_cli_bgzf_report_takes_the_report_route(cli_work):
    d, truth, _, n_rep = cli_work
    p = cli(["-i", d / "bgzf.yacrd.gz", "-o", d / "f.yacrd"])
    assert report_set(d / "f.yacrd") == truth
    inf = stderr_lines(p, "[info] device inflate:")
    assert len(inf) == 1 and (" -> %d bytes" % n_rep) in inf[0], p.stderr
    rd = stderr_lines(p, "[info] device report reader:")
    assert len(rd) == 1 and "230 reads from 230 lines" in rd[0] and "(inflated in HBM)" in rd[0]
    assert "[timing] inflate" not in p.stderr
    q = cli(["-i", d / "bgzf.yacrd.gz", "-o", d / "g.yacrd"], YACRD_NO_DEVICE_INFLATE="1")
    assert (d / "g.yacrd").read_bytes() == (d / "f.yacrd").read_bytes()
    assert "[timing] inflate" in q.stderr and not stderr_lines(q, "[info] device inflate:")
