"""A BGZF FASTQ / FASTA edited window by window (csrc/gpu_seq_edit.hip: run_windows with inflate_window; csrc/gpu_inflate.hip:
inf_window_kernel): the windows end where members end, every window's members are inflated into its text slot, and
the bytes do not change.  The yardsticks: the restatements and the host loop (pinned on the CPU), Engine.gzip of the plain
bytes, the cut rule (host.bgzf_window_cuts, pinned to tests/edit_bgzf_window_cases.py: member_cuts) and the run restated for
windows that end anywhere (window_carries_at).  Every test asserts the windows the edit reports against the cuts and its
longest carry against the restatement: none passes on the whole-text route."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import edit_fasta_cases as fa
import edit_fasta_window_cases as faw
import edit_fastq_cases as fq
import edit_fastq_window_cases as fqw
import inflate_cases as ic
import yacrd_amd
from deflate_cases import EOF_MEMBER
from edit_bgzf_window_cases import W_BGZF, borders_of, drawn_stream, frames_of, stream_of, window_carries_at
from edit_fastq_cases import CHIMERIC, OPS, OP_EXTRACT, OP_FILTER, OP_SCRUBB, OP_SPLIT, Table
from yacrd_amd import engine as engine_module
from yacrd_amd import host
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
W = W_BGZF
_BLOCK = 65280
_NEVER = 2 ** 64 - 1
_LONGER = "a record longer than a window"
_MOD = {"fastq": (fq, fqw), "fasta": (fa, faw)}


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e
        e.debug_seq_window(0)


@pytest.fixture(scope="module")
def generated():
    """fmt -> (text, table, blob): about 20 windows of text in members of drawn sizes and kinds"""
    out = {}
    for fmt, seed in (("fastq", 1000), ("fasta", 2000)):
        table = _MOD[fmt][1].window_table()
        text = _MOD[fmt][1].window_text(table, seed, 20 * W)
        out[fmt] = (text, table, drawn_stream(text, 11)[0])
    return out


def _chunks(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def _edit(engine, fmt, op, blob, table, out_path=None):
    names, lengths, bo, br, rt = table.arrays()
    return getattr(engine, "edit_%s_bgzf" % fmt)(op, blob, names, lengths, (bo, br, rt), out_path=out_path)


def _ran_as(engine, fmt, text, blob, w=W):
    """the last edit ran in the windows the cut rule gives and carried what the restatement carries -> (cuts, carries)"""
    cuts = host.bgzf_window_cuts(blob, w)
    carries = window_carries_at(text, borders_of(cuts), fmt == "fasta", w)
    sw = engine.seq_windows()
    assert len(cuts) > 1 and sw["windows"] == len(cuts), (sw, len(cuts))
    assert carries is not None and sw["max_carry"] == max(carries), (sw, max(carries))
    assert sw["text_ring_bytes"] >= 2 * (2 * w + 64) + w + 64
    us = engine.gunzip_stats
    assert (us["in_bytes"], us["out_bytes"], us["n_members"]) == (len(blob), len(text), len(frames_of(blob)[0]))
    return cuts, carries


def _windows_give(engine, fmt, op, text, blob, table, plain=None, whole=True):
    """the edit in windows of W: the bytes Engine.gzip makes of the restated plain bytes, and the whole-text run's"""
    plain = _MOD[fmt][0].restate(text, op, table)[0] if plain is None else plain
    engine.debug_seq_window(W)
    got = _edit(engine, fmt, op, blob, table)
    ran = _ran_as(engine, fmt, text, blob)
    assert gzip.decompress(got) == plain
    assert got == engine.gzip(plain)
    assert engine.seq_edit_stats["text_bytes"] == len(text) and engine.seq_edit_stats["out_bytes"] == len(plain)
    if whole:
        engine.debug_seq_window(_NEVER)
        assert _edit(engine, fmt, op, blob, table) == got and engine.seq_windows()["windows"] == 0
        engine.debug_seq_window(W)
    return got, ran


# ---- 1: generated texts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_generated_texts_all_four_ops_mem_and_file(engine, generated, tmp_path, fmt):
    text, table, blob = generated[fmt]
    for op in OPS:
        got, _ = _windows_give(engine, fmt, op, text, blob, table)
        out = tmp_path / "out.gz"
        es, gs = _edit(engine, fmt, op, blob, table, out_path=str(out))
        _ran_as(engine, fmt, text, blob)
        assert out.read_bytes() == got and es["text_bytes"] == len(text) and gs["out_bytes"] == len(got), op
        assert os.listdir(tmp_path) == ["out.gz"]
        out.unlink()


# ---- 2: window borders against record borders -------------------------------------------------------------------------------------
_TARGETS = {
    "fastq": b"@target of the cut\n" + b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\n" + b"#" * 40 + b"\n",
    "fasta": b">target of the cut\n" + b"ACGTACGTACGTACGTA\n" + b"CGTACG\n" + b"\n" + b"TACGTACGTACGTACGT\n",
}
_TARGET_TABLE = Table([b"target"], [40], [[(5, 10), (20, 21)]], [CHIMERIC])


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_border_sweep(engine, fmt):
    """every byte of a cut record is the first new byte of window 1 (FASTA: the newline in front of its '>' too); where window 0
    ends is the first member's size, another for each op"""
    mod = _MOD[fmt][1]
    target = _TARGETS[fmt]
    for op, first in ((OP_SCRUBB, 60000), (OP_SPLIT, 50001)):
        for before in range(-1 if fmt == "fasta" else 0, len(target), 1 if op == OP_SCRUBB else 3):  # (split: every third byte)
            text = mod.fillers(first - before) + target + mod.fillers(W // 2)
            assert text[first - before:].startswith(target) and text[first:first + 1] == (target[before:before + 1] if before >= 0 else b"\n")
            blob = stream_of(text, [first] + _chunks(len(text) - first, 30000), "level1")
            cuts = host.bgzf_window_cuts(blob, W)
            assert cuts[0][5] == first and len(text) > W
            got, (_, carries) = _windows_give(engine, fmt, op, text, blob, _TARGET_TABLE, whole=False)
            assert carries[0] >= max(before, 0), (before, carries)


# ---- 3: the windows' edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_a_window_of_exactly_w_bytes_of_text_and_the_compressed_cap(engine, generated, fmt):
    text, table, _ = generated[fmt]
    text = text[:text.rindex(b"\n@f\n" if fmt == "fastq" else b"\n>", 0, 6 * W) + 1]
    blob = stream_of(text, [32768, 32768] + _chunks(len(text) - W, 65536), "level6")
    assert host.bgzf_window_cuts(blob, W)[0][4:] == (0, W)
    _windows_give(engine, fmt, OP_SCRUBB, text, blob, table)
    # two stored members of 32 760 bytes: 65 520 bytes of text fit a window, their 65 582 bytes of frames do not
    sizes = [32760, 32760] + _chunks(len(text) - 65520, 50000)
    blob = stream_of(text, sizes, ["stored", "stored"] + ["level1"] * (len(sizes) - 2))
    assert host.bgzf_window_cuts(blob, W)[0] == (0, 1, 0, 32791, 0, 32760)
    _windows_give(engine, fmt, OP_SCRUBB, text, blob, table)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_a_run_of_eof_members_mid_text(engine, generated, fmt):
    """a stored member of 65 505 bytes fills a window's frames; 3 000 EOF members behind it are windows with no new bytes, and
    the record the member cut lies in their carry"""
    text, table, _ = generated[fmt]
    text = text[:text.rindex(b"\n@f\n" if fmt == "fastq" else b"\n>", 0, 5 * W) + 1]
    sizes = [60000, 65505] + [0] * 3000 + _chunks(len(text) - 125505, 65536)
    blob = stream_of(text, sizes, ["level1", "stored"] + ["level1"] * (len(sizes) - 2))
    for op in (OP_SCRUBB, OP_FILTER):
        _, (cuts, carries) = _windows_give(engine, fmt, op, text, blob, table, whole=op == OP_SCRUBB)
        empty = [k for k, c in enumerate(cuts) if c[4] == c[5]]
        assert len(empty) >= 1 and all(0 < k < len(cuts) - 1 and carries[k] > 0 and carries[k] == carries[k - 1] for k in empty)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_a_last_window_with_no_new_bytes(engine, generated, fmt):
    """the text's last member is stored and fills a window's frames: the EOF member behind it is the last window, of no bytes.
    FASTQ: nothing is left for it.  FASTA: the window before could not know that its last record was whole; this one completes it"""
    text, table, _ = generated[fmt]
    text = text[:text.rindex(b"\n@f\n" if fmt == "fastq" else b"\n>", 0, 4 * W) + 1]
    sizes = _chunks(len(text) - 65505, 65536) + [65505]
    blob = stream_of(text, sizes, ["level6"] * (len(sizes) - 1) + ["stored"])
    for op in (OP_SCRUBB, OP_EXTRACT):
        _, (cuts, carries) = _windows_give(engine, fmt, op, text, blob, table)
        assert cuts[-1][4] == cuts[-1][5] == len(text) and (carries[-1] > 0) == (fmt == "fasta")


def _right_or_the_host_loops(engine, fmt, op, text, blob, table):
    cuts = host.bgzf_window_cuts(blob, W)
    if window_carries_at(text, borders_of(cuts), fmt == "fasta", W) is None:
        engine.debug_seq_window(W)
        with pytest.raises(yacrd_amd.NeedsHostParser, match=_LONGER):
            _edit(engine, fmt, op, blob, table)
        assert engine.seq_windows()["windows"] == 0
        return None
    return _windows_give(engine, fmt, op, text, blob, table, whole=False)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("sizes", [(W - 5,), (W + 15,), (W - 5, W + 15)], ids=["records_of_W-5", "records_of_W+15", "both_in_turn"])
def test_carry_chain(engine, fmt, sizes):
    """records of W - 5 and of W + 15 bytes back to back, in members of 65 536 and of 40 000 bytes of text: taken where the
    restatement goes through, handed to the host loop where a carry outgrows its area — never other bytes"""
    mod = _MOD[fmt][1]
    text = mod.fillers(W - 5) + b"".join(mod.record_of(sizes[i % len(sizes)], b"c%02d" % i) for i in range(10)) + mod.filler(55)
    took = []
    for each in (65536, 40000):
        blob = stream_of(text, _chunks(len(text), each), "level1")
        took.append(_right_or_the_host_loops(engine, fmt, OP_FILTER, text, blob, Table()) is not None)
    assert max(sizes) > W or all(took)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_a_record_of_two_windows_and_a_byte_falls_back(engine, fmt):
    text = _MOD[fmt][1].long_record_text(W)
    blob = stream_of(text, _chunks(len(text), 65536), "level1")
    assert _right_or_the_host_loops(engine, fmt, OP_FILTER, text, blob, Table()) is None
    engine.debug_seq_window(_NEVER)
    assert gzip.decompress(_edit(engine, fmt, OP_FILTER, blob, Table())) == _MOD[fmt][0].restate(text, OP_FILTER, Table())[0]


# ---- 4: causes found late --------------------------------------------------------------------------------------------------------
def _mem_form_raw(engine, fmt, op, blob, table):
    """yacrd_engine_edit_<fmt>_bgzf_mem as C sees it -> (code, the buffer's address, its bytes, the three stats)"""
    names, lengths, bo, br, rt = table.arrays()
    t, keep = engine._seq_table(names, lengths, (bo, br, rt))
    st, gs, us = engine_module._SeqEditStats(), engine_module._GzipStats(), engine_module._GunzipStats()
    buf = np.frombuffer(blob, dtype=np.uint8)
    out, n_out = ctypes.c_void_p(), ctypes.c_uint64(77)
    rc = getattr(engine._lib, "yacrd_engine_edit_%s_bgzf_mem" % fmt)(engine._h, int(op), ctypes.c_void_p(buf.ctypes.data), int(buf.size), t,
                                                                     ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(gs),
                                                                     ctypes.byref(us))
    del keep
    stats = [getattr(s, n) for s in (st, gs, us) for n, _ in s._fields_]
    return rc, out.value, int(n_out.value), stats


def _falls_back_everywhere(engine, tmp_path, fmt, op, blob, table, cause, walked=True):
    d = tmp_path / "dev"
    d.mkdir(exist_ok=True)
    out = d / ("out.%s.gz" % fmt)
    out.write_bytes(b"what was there")
    engine.debug_seq_window(W)
    with pytest.raises(yacrd_amd.NeedsHostParser, match=cause):
        _edit(engine, fmt, op, blob, table)
    assert not walked or engine.seq_windows()["windows"] == 0  # (what the walk refuses never reaches the run that reports)
    rc, addr, n_out, stats = _mem_form_raw(engine, fmt, op, blob, table)
    assert rc == engine_module.E_FALLBACK and not addr and n_out == 0 and not any(stats), (rc, addr, n_out, stats)
    for path in (out, d / "new.gz"):
        with pytest.raises(yacrd_amd.NeedsHostParser, match=cause):
            _edit(engine, fmt, op, blob, table, out_path=str(path))
        assert os.listdir(d) == [out.name] and out.read_bytes() == b"what was there"


def _late_causes(fmt, good):
    """(tag, text', damage: a function of the stream or None, the cause in the message)"""
    at = good.index(b"\n", 3 * W + W // 2)
    out = [("a damaged CRC", good, "crc", "CRC mismatch"), ("a CR", good[:at] + b"\r" + good[at:], None, "CR")]
    if fmt == "fastq":
        out.append(("a deleted line", good[:at] + good[good.index(b"\n", at + 1):], None, "the host loop decides"))
    else:
        out.append(("a base line in front of the first header", b"ACGT\n" + good, None, "bases in front of the first header"))
    return out


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_fallback_causes_behind_three_good_windows(engine, tmp_path, fmt):
    mod, wmod = _MOD[fmt]
    table = wmod.window_table()
    good = wmod.window_text(table, 7, 5 * W)
    sizes = _chunks(len(good), 60000)
    _windows_give(engine, fmt, OP_FILTER, good, stream_of(good, sizes, "level1"), table, whole=False)
    for tag, text, damage, cause in _late_causes(fmt, good):
        members = [ic.member(text[i:i + 60000], 1) for i in range(0, len(text), 60000)]
        if damage == "crc":  # the fifth member: three whole windows lie in front of it, and it is not the one the host looks at
            bad = bytearray(members[4])
            bad[-8] ^= 1
            members[4] = bytes(bad)
        blob = b"".join(members) + EOF_MEMBER
        assert len(host.bgzf_window_cuts(blob, W)) >= 5, tag
        _falls_back_everywhere(engine, tmp_path, fmt, OP_FILTER, blob, table, cause)
        # the engine goes on
        _windows_give(engine, fmt, OP_SCRUBB, good, stream_of(good, sizes, "level1"), table, whole=False)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_refused_before_the_first_window(engine, tmp_path, fmt):
    """a missing final newline and a last member the host decoder refuses are found before anything is launched or written;
    plain gzip and the framings that are not BGZF are refused as before"""
    wmod = _MOD[fmt][1]
    good = wmod.fillers(4 * W)
    sizes = _chunks(len(good), 60000)
    _windows_give(engine, fmt, OP_FILTER, good, stream_of(good, sizes, "level1"), Table(), whole=False)
    _falls_back_everywhere(engine, tmp_path, fmt, OP_FILTER, stream_of(good[:-1], _chunks(len(good) - 1, 60000), "level1"), Table(), "no newline")
    last = bytearray(stream_of(good, sizes, "level1", eof=False))
    last[-8] ^= 1  # the last member's CRC
    _falls_back_everywhere(engine, tmp_path, fmt, OP_FILTER, bytes(last) + EOF_MEMBER, Table(), "CRC mismatch")
    _falls_back_everywhere(engine, tmp_path, fmt, OP_FILTER, gzip.compress(good, 1), Table(), "not BGZF", walked=False)
    for tag, blob in ic.not_bgzf_cases():
        with pytest.raises(yacrd_amd.NeedsHostParser, match="not BGZF"):
            _edit(engine, fmt, OP_FILTER, blob, Table())
    _windows_give(engine, fmt, OP_FILTER, good, stream_of(good, sizes, "level1"), Table(), whole=False)


# ---- 5: bounded memory -----------------------------------------------------------------------------------------------------------
def test_the_device_holds_a_ring_not_the_text_or_the_stream():
    """the same records in 8 and in 64 windows: what the editor holds behind the edit does not grow with the text.  The bound:
    two text slots of 2 W, the compressed slot of W, two output slots of at most 2 W, the member slice, the tables per record
    and per tile in the slack, the encoder's slots by the batch"""
    rec = fqw.filler(1019)
    with yacrd_amd.Engine(device_id=0) as e:
        e.debug_seq_window(W)
        _edit(e, "fastq", OP_FILTER, ic.bgzf_of(rec * 200, chunk=65536, level=1), Table())
        e.trim()
        start = live_bytes()[0]
        held = {}
        for n_win in (8, 64):
            text = rec * (n_win * W // len(rec))
            blob = ic.bgzf_of(text, chunk=65536, level=1)
            assert gzip.decompress(_edit(e, "fastq", OP_FILTER, blob, Table())) == text
            _ran_as(e, "fastq", text, blob)
            w = e.seq_windows()
            assert w["windows"] == n_win
            held[n_win] = live_bytes()[0]
            print("held behind %d windows: %d bytes (ring %d + %d)" % (n_win, held[n_win] - start, w["text_ring_bytes"], w["out_ring_bytes"]))
            assert held[n_win] - start < 11 * W + (4 << 20)
            assert w["text_ring_bytes"] + w["out_ring_bytes"] <= held[n_win] - start
            e.trim()
            assert live_bytes()[0] == start
        assert held[64] <= held[8]


# ---- 6: gzip out -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("k", [0, 2])
def test_gzip_a_windows_output_ends_at_a_block_border(engine, tmp_path, k, d):
    """fillers go out as they came in: the records window k completes end a byte before, on and a byte behind a border of the
    output's 65 280-byte blocks, and the windows' ends drift against the blocks from there"""
    end = (k + 1) * _BLOCK + d
    text = fqw.fillers(end) + fqw.fillers(5 * W + 777)
    blob = stream_of(text, _chunks(len(text), 65536), "level1")
    assert fq.restate(text, OP_FILTER, Table())[0] == text
    got, (cuts, carries) = _windows_give(engine, "fastq", OP_FILTER, text, blob, Table(), plain=text, whole=False)
    assert borders_of(cuts)[k] == (k + 1) * W and carries[k] == (k + 1) * W - end
    assert engine.gzip_stats["in_bytes"] == len(text) and engine.gzip_stats["n_members"] == (len(text) + _BLOCK - 1) // _BLOCK
    es, gs = _edit(engine, "fastq", OP_FILTER, blob, Table(), out_path=str(tmp_path / "o.fastq.gz"))
    assert (tmp_path / "o.fastq.gz").read_bytes() == got and os.listdir(tmp_path) == ["o.fastq.gz"]
    assert es["out_bytes"] == len(text) == gs["in_bytes"] and gs["out_bytes"] == len(got)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_gzip_a_window_that_keeps_nothing_and_nothing_at_all(engine, fmt):
    wmod = _MOD[fmt][1]
    drop = b"@gone\n" + b"ACGT" * 100 + b"\n+\n" + b"#" * 400 + b"\n" if fmt == "fastq" else b">gone\n" + (b"ACGT" * 20 + b"\n") * 5
    table = Table([b"gone"], [400], [[(10, 20)]], [CHIMERIC])
    text = wmod.fillers(W + W // 2) + drop * (3 * W // len(drop) + 2) + wmod.fillers(W + 99)
    kept = text.replace(drop, b"")
    blob = stream_of(text, _chunks(len(text), 65536), "level6")
    first = text.index(drop)
    assert first < 2 * W and first + 2 * W < text.rindex(drop)  # (a window holds dropped records alone)
    _windows_give(engine, fmt, OP_FILTER, text, blob, table, plain=kept)
    _windows_give(engine, fmt, OP_SCRUBB, text, blob, table)
    text = wmod.fillers(3 * W + 5)
    got, _ = _windows_give(engine, fmt, OP_EXTRACT, text, stream_of(text, _chunks(len(text), 65536), "level1"), Table(), plain=b"")
    assert got == EOF_MEMBER


# ---- 7: the CLI ------------------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_cli_in_windows_on_a_generated_bgzf_file(generated, tmp_path, fmt):
    """the command on a generated BGZF file and a report of the generator's table: under YACRD_SEQ_WINDOW=65536 the editor's
    line ends in windows=K, K the cuts', and the file is the one the run without the variable writes"""
    text, table, blob = generated[fmt]
    src, rep = tmp_path / ("gen.%s.gz" % fmt), tmp_path / "gen.yacrd"
    src.write_bytes(blob)
    kinds = ("NotBad", "Chimeric", "NotCovered")
    rep.write_bytes(b"".join(b"%s\t%s\t%d\t%s\n" % (kinds[t].encode(), n, l, b";".join(b"%d,%d,%d" % (e - b, b, e) for b, e in r))
                             for n, l, r, t in zip(table.names, table.lengths, table.regions, table.types)))
    a, b = tmp_path / ("win.%s.gz" % fmt), tmp_path / ("whole.%s.gz" % fmt)
    p = _cli(["-i", rep, "-o", tmp_path / "r.yacrd", "-n", "0.8", "scrubb", "-i", src, "-o", a], YACRD_CLI_TIMING="1", YACRD_SEQ_WINDOW="65536")
    assert p.returncode == 0, p.stderr
    line = [l for l in p.stderr.splitlines() if l.startswith("[info] device %s editor:" % fmt)]
    assert len(line) == 1 and int(line[0].rsplit("windows=", 1)[1]) == len(host.bgzf_window_cuts(blob, W)) > 1, p.stderr
    assert len([l for l in p.stderr.splitlines() if l.startswith("[info] device inflate:")]) == 1, p.stderr
    q = _cli(["-i", rep, "-o", tmp_path / "r2.yacrd", "-n", "0.8", "scrubb", "-i", src, "-o", b], YACRD_CLI_TIMING="1")
    assert q.returncode == 0, q.stderr
    line = [l for l in q.stderr.splitlines() if l.startswith("[info] device %s editor:" % fmt)]
    assert len(line) == 1 and line[0].endswith("windows=0"), q.stderr
    assert a.read_bytes() == b.read_bytes() and len(gzip.decompress(a.read_bytes())) > 1000
