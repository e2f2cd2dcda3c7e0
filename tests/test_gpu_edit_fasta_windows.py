"""The FASTA editor window by window (csrc/gpu_seq_edit.hip: run_windows): a text of more than one window is edited
in a bounded ring of buffers, and the bytes do not change.  The yardsticks are the restatement and the host loop
(tests/edit_fasta_cases.py, pinned on the CPU), the windows' own rule (tests/edit_fasta_window_cases.py) and engine.gzip of the
plain bytes — never the whole-text run.  Every test reads seq_windows()["windows"]: none passes on the whole-text route."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import yacrd_amd
from edit_fasta_cases import BASES_FIRST, CHIMERIC, OPS, OP_EXTRACT, OP_FILTER, OP_SCRUBB, OP_SPLIT, Table, fallback_cases, host_loop, restate
from edit_fasta_window_cases import (W_SMALL, blank_front_text, filler, fillers, long_record_text, n_windows, record_of, window_carries,
                                     window_cases, window_table, window_text, windows_take)
from yacrd_amd import engine as engine_module
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
_BLOCK = 65280     # bytes of text per BGZF member (csrc/bgzf_sizes.h: kBlock)
_EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_NEVER = 2 ** 64 - 1
_LONGER = "a record longer than a window"


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e
        e.debug_seq_window(0)


@pytest.fixture(scope="module")
def cases():
    return list(window_cases())


def _edit(engine, op, text, table):
    names, lengths, bo, br, rt = table.arrays()
    return engine.edit_fasta_text(op, text, names, lengths, (bo, br, rt))


def _gz(engine, op, text, table, out_path=None):
    names, lengths, bo, br, rt = table.arrays()
    return engine.edit_fasta_gzip(op, text, names, lengths, (bo, br, rt), out_path=out_path)


def _ran_as(engine, text, W):
    """the last edit ran in the windows the rule gives, and carried what the restatement carries"""
    w = engine.seq_windows()
    assert w["windows"] == n_windows(text, W), w
    if w["windows"]:
        assert w["max_carry"] == max(window_carries(text, W)) and w["text_ring_bytes"] >= 2 * (2 * W + 64), w
    return w


# ---- 1: generated texts ---------------------------------------------------------------------------------------------------------
def test_generated_texts_all_four_ops(engine, cases, tmp_path):
    for tag, text, table in cases:
        assert windows_take(text, W_SMALL) is True and n_windows(text, W_SMALL) >= 40
        for op in OPS:
            want, n_in, n_out = restate(text, op, table)
            engine.debug_seq_window(W_SMALL)
            assert _edit(engine, op, text, table) == want, (tag, op)
            _ran_as(engine, text, W_SMALL)
            st = engine.seq_edit_stats
            assert (st["text_bytes"], st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(text), len(want), n_in, n_out), (tag, op)
            if op == OP_SCRUBB:
                assert want == host_loop(str(tmp_path), op, text, table, ext=".fasta"), tag
            engine.debug_seq_window(_NEVER)
            assert _edit(engine, op, text, table) == want and engine.seq_windows()["windows"] == 0, (tag, op)


# ---- 2: every byte of a cut record as the first byte of window 1 -----------------------------------------------------------------
_TARGET = b">target of the cut\n" + b"ACGTACGTACGTACGTA\n" + b"CGTACG\n" + b"\n" + b"TACGTACGTACGTACGT\n"  # 40 bases on three ragged lines, a blank one
_TARGET_TABLE = Table([b"target"], [40], [[(5, 10), (20, 21)]], [CHIMERIC])


def test_border_sweep(engine, tmp_path):
    """two windows; byte `before` of the cut record is the first new byte of window 1 — the newline in front of its '>'
    (before = -1), the '>', every byte of the header and its newline, every base, the blank line —: every line of the
    record crosses the border, and so does the decision whether the record in front of it was whole"""
    W = W_SMALL
    engine.debug_seq_window(W)
    wants = {}
    for before in range(-1, len(_TARGET)):
        text = fillers(W - before) + _TARGET + fillers(W // 2)
        assert text[W - before:].startswith(_TARGET) and W < len(text) <= 2 * W
        assert text[W:W + 1] == (_TARGET[before:before + 1] if before >= 0 else b"\n")
        for op in (OP_SCRUBB, OP_SPLIT):
            want = restate(text, op, _TARGET_TABLE)[0]
            assert _edit(engine, op, text, _TARGET_TABLE) == want, (before, op)
            w = engine.seq_windows()
            assert w["windows"] == 2 and w["max_carry"] == max(window_carries(text, W)), (before, w)
            wants[op] = (text, want)
    text, want = wants[OP_SCRUBB]
    assert want == host_loop(str(tmp_path), OP_SCRUBB, text, _TARGET_TABLE, ext=".fasta") and b">target_0_5\nACGTA\n>target_10_20\n" in want


# ---- 3: a record that ends with its window waits all the same --------------------------------------------------------------------
def test_a_complete_record_at_a_windows_end_is_deferred(engine):
    """window 0 ends exactly behind the record's last newline and window 1 begins with '>': nothing in window 0 says so, the
    record is carried whole and leaves with window 1"""
    W = W_SMALL
    rec = record_of(700, b"ends", width=60, desc=b"with its window")
    table = Table([b"ends"], [600], [[(100, 200)]], [CHIMERIC])
    text = fillers(W - 700) + rec + fillers(W // 2)
    assert text[W - 700:W] == rec and text[W:W + 2] == b">f" and window_carries(text, W) == [700]
    engine.debug_seq_window(W)
    for op in OPS:
        assert _edit(engine, op, text, table) == restate(text, op, table)[0], op
        w = _ran_as(engine, text, W)
        assert w["windows"] == 2 and w["max_carry"] == len(rec)
    # a byte later the next record's '>' is in the window: the record is whole there, and only that byte waits
    text = fillers(W - 701) + rec + fillers(W // 2)
    assert window_carries(text, W) == [1]
    assert _edit(engine, OP_SCRUBB, text, table) == restate(text, OP_SCRUBB, table)[0] and _ran_as(engine, text, W)["max_carry"] == 1


# ---- 4: the carry ----------------------------------------------------------------------------------------------------------------
def _right_or_the_host_loops(engine, op, text, table, W):
    """right bytes in windows where the window-by-window restatement goes through, the fallback of DESIGN 7k where it does
    not; never other bytes"""
    carries = window_carries(text, W)
    took = windows_take(text, W)
    assert (took is not True or carries is not None) and (took is not False or carries is None)
    if carries is None:
        with pytest.raises(yacrd_amd.NeedsHostParser, match=_LONGER):
            _edit(engine, op, text, table)
        assert engine.seq_windows()["windows"] == 0
        return None
    assert _edit(engine, op, text, table) == restate(text, op, table)[0], op
    return _ran_as(engine, text, W)


@pytest.mark.parametrize("sizes", [(W_SMALL - 5,), (W_SMALL + 15,), (W_SMALL - 5, W_SMALL + 15)], ids=["records_of_W-5", "records_of_W+15", "both_in_turn"])
@pytest.mark.parametrize("first", [W_SMALL - 5, W_SMALL + 15], ids=["from_W-5", "from_W+15"])
def test_carry_chain(engine, first, sizes):
    """records of W - 5 bytes back to back: every window completes one record at the most and carries what it holds of the
    next — a few bytes more with every window, or from W + 15 on nearly a whole record —; all are taken.  Records of W + 15 bytes, alone and in turn with the others: the
    rule leaves them to the run, which takes the text or hands it to the host loop as the restatement says"""
    W = W_SMALL
    text = fillers(first) + b"".join(record_of(sizes[i % len(sizes)], b"c%02d" % i, width=70) for i in range(12)) + filler(55)
    assert windows_take(text, W) is (True if max(sizes) <= W else None)
    engine.debug_seq_window(W)
    for op in (OP_SCRUBB, OP_FILTER, OP_EXTRACT):
        w = _right_or_the_host_loops(engine, op, text, Table(), W)
        assert max(sizes) > W or (w is not None and w["max_carry"] > 0)  # (the carries themselves: _ran_as against window_carries)


# ---- 5: record sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, W_SMALL + 1, 2 * W_SMALL - 1])
def test_a_record_of_exactly_a_window_is_taken(engine, at):
    """at offsets 0, 1 and W - 1 of a window; at W - 1 the window behind ends with the next record's '>'"""
    W = W_SMALL
    text = (fillers(at) if at else b"") + record_of(W, b"bg") + filler(33)
    assert windows_take(text, W) is True and text[at:].startswith(b">bg") and text[at + W:].startswith(b">f")
    engine.debug_seq_window(W)
    table = Table([b"bg" if text[at + 3:at + 4] == b"\n" else b"bgx"], [W - 500], [[(7, 9), (81, 30000)]], [CHIMERIC])
    for op in OPS:
        want = restate(text, op, table)[0]
        assert _edit(engine, op, text, table) == want, op
        _ran_as(engine, text, W)
    assert b"_9_81\n" in restate(text, OP_SCRUBB, table)[0]


def test_a_record_of_two_windows_and_a_byte_falls_back(engine):
    W = W_SMALL
    engine.debug_seq_window(W)
    with pytest.raises(yacrd_amd.NeedsHostParser, match=_LONGER):
        _edit(engine, OP_FILTER, long_record_text(W), Table())
    assert engine.seq_windows()["windows"] == 0
    engine.debug_seq_window(_NEVER)
    assert _edit(engine, OP_FILTER, long_record_text(W), Table()) == long_record_text(W)


# ---- 6: a window of very many lines ----------------------------------------------------------------------------------------------
def test_a_record_at_width_one(engine):
    """W - 64 bytes at one base a line: the window that holds it has about W / 2 lines — the line tables are sized by the
    measured count, a window's first reserve grows them tenfold"""
    W = W_SMALL
    rec = record_of(W - 64, b"thin", width=1, desc=b"one base a line")
    n = rec.count(b"\n") - 1
    table = Table([b"thin"], [n], [[(3, 5), (1000, 1001), (n - 7, n)]], [CHIMERIC])
    text = fillers(2 * W + 300) + rec + fillers(W + 77)
    assert n > W // 2 - 64 and windows_take(text, W) is True
    engine.debug_seq_window(W)
    for op in OPS:
        assert _edit(engine, op, text, table) == restate(text, op, table)[0], op
        _ran_as(engine, text, W)


# ---- 7: lines in front of the first header ---------------------------------------------------------------------------------------
def test_blank_lines_in_front_of_the_first_header_span_a_border(engine):
    W = W_SMALL
    text = blank_front_text(W, tail=fillers(W + 5))
    table = Table([b"first"], [6], [[(2, 3)]], [CHIMERIC])
    assert windows_take(text, W) is True and window_carries(text, W)[0] == W
    engine.debug_seq_window(W)
    for op in OPS:
        assert _edit(engine, op, text, table) == restate(text, op, table)[0], op
        assert _ran_as(engine, text, W)["max_carry"] == W
    assert restate(text, OP_SCRUBB, table)[0].startswith(b">first_0_2\nAC\n>first_3_6\n")


def test_more_than_two_windows_in_front_of_the_first_header_fall_back(engine):
    """2 W blank lines and then the header: window 1 holds no whole header line and would carry 2 W bytes.  The message says
    what happened — no record was too long"""
    W = W_SMALL
    text = b"\n" * (2 * W) + b">r\nAC\n" + fillers(W)
    assert windows_take(text, W) is False and window_carries(text, W) is None
    engine.debug_seq_window(W)
    with pytest.raises(yacrd_amd.NeedsHostParser, match="in front of the first header's newline"):
        _edit(engine, OP_FILTER, text, Table())
    assert engine.seq_windows()["windows"] == 0
    engine.debug_seq_window(_NEVER)
    assert _edit(engine, OP_FILTER, text, Table()) == text[2 * W:]


@pytest.mark.parametrize("front", BASES_FIRST + [b"\n" * 9 + b"ACGT\n"], ids=["bases", "blank_then_a_base", "a_blank", "blanks_then_bases"])
def test_a_base_line_in_front_of_the_first_header_falls_back(engine, front):
    W = W_SMALL
    engine.debug_seq_window(W)
    assert _edit(engine, OP_FILTER, fillers(3 * W), Table()) == fillers(3 * W) and engine.seq_windows()["windows"] == 3
    with pytest.raises(yacrd_amd.NeedsHostParser, match="bases in front of the first header"):
        _edit(engine, OP_FILTER, front + fillers(3 * W), Table())
    assert engine.seq_windows()["windows"] == 0


# ---- 8: causes found late -------------------------------------------------------------------------------------------------------
def _mem_form_raw(engine, op, text, table):
    """yacrd_engine_edit_fasta_mem as C sees it -> (code, the buffer's address, its bytes, the stats)"""
    names, lengths, bo, br, rt = table.arrays()
    t, keep = engine._seq_table(names, lengths, (bo, br, rt))
    st = engine_module._SeqEditStats()
    buf = np.frombuffer(text, dtype=np.uint8)
    out, n_out = ctypes.c_void_p(), ctypes.c_uint64(77)
    rc = engine._lib.yacrd_engine_edit_fasta_mem(engine._h, int(op), ctypes.c_void_p(buf.ctypes.data), int(buf.size), t, ctypes.byref(out),
                                                 ctypes.byref(n_out), ctypes.byref(st))
    del keep
    return rc, out.value, int(n_out.value), {n: getattr(st, n) for n, _ in engine_module._SeqEditStats._fields_}


def _falls_back_everywhere(engine, tmp_path, op, text, table):
    d = tmp_path / "dev"
    d.mkdir(exist_ok=True)
    src, out = tmp_path / "in.fasta", d / "out.fasta"
    src.write_bytes(text)
    out.write_bytes(b"what was there")
    names, lengths, bo, br, rt = table.arrays()
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _edit(engine, op, text, table)
    assert engine.seq_windows()["windows"] == 0
    rc, addr, n_out, st = _mem_form_raw(engine, op, text, table)
    assert rc == engine_module.E_FALLBACK and not addr and n_out == 0 and not any(st.values()), (rc, addr, n_out, st)
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.edit_fasta(op, str(src), str(out), names, lengths, (bo, br, rt))
    assert os.listdir(d) == ["out.fasta"] and out.read_bytes() == b"what was there"
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _gz(engine, op, text, table, out_path=str(d / "out.fasta.gz"))
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _gz(engine, op, text, table, out_path=str(out))
    assert os.listdir(d) == ["out.fasta"] and out.read_bytes() == b"what was there"


_FALLBACKS = fallback_cases()


@pytest.mark.parametrize("tag,ops,bad,table", _FALLBACKS, ids=[f[0] for f in _FALLBACKS])
def test_fallback_causes_behind_three_good_windows(engine, tmp_path, tag, ops, bad, table):
    W = W_SMALL
    good = window_text(window_table(), 7, 3 * W + 100)  # (reads the case's table does not hold: copied, or dropped by extract)
    engine.debug_seq_window(W)
    assert _edit(engine, ops[0], good, table) == restate(good, ops[0], table)[0] and engine.seq_windows()["windows"] == n_windows(good, W) >= 4
    _falls_back_everywhere(engine, tmp_path, ops[0], good + bad, table)


# ---- 9: gzip out ----------------------------------------------------------------------------------------------------------------
def _gzip_is(engine, op, text, table, plain):
    W = 65536
    engine.debug_seq_window(W)
    assert _edit(engine, op, text, table) == plain
    blob = _gz(engine, op, text, table)
    _ran_as(engine, text, W)
    assert gzip.decompress(blob) == plain
    assert blob == engine.gzip(plain)
    assert engine.gzip_stats["in_bytes"] == len(plain) and engine.gzip_stats["n_members"] == (len(plain) + _BLOCK - 1) // _BLOCK  # (the EOF member is not counted)
    return blob


@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("k", [0, 2])
def test_gzip_a_windows_output_ends_at_a_block_border(engine, tmp_path, k, d):
    """the fillers go out as they came in, so the restatement's lengths are the text's: the records window k completes end
    a byte before, on and a byte behind a border of the 65 280-byte blocks — the record behind them lies across the
    window's end —, and the windows' ends drift against the blocks from there"""
    W = 65536
    end = (k + 1) * _BLOCK + d
    text = fillers(end) + fillers(5 * W + 777)
    assert restate(text, OP_FILTER, Table())[0] == text and len(restate(fillers(end), OP_FILTER, Table())[0]) == end
    assert k * W < end <= (k + 1) * W and window_carries(text, W)[k] == (k + 1) * W - end
    blob = _gzip_is(engine, OP_FILTER, text, Table(), text)
    es, gs = _gz(engine, OP_FILTER, text, Table(), out_path=str(tmp_path / "o.fasta.gz"))
    assert (tmp_path / "o.fasta.gz").read_bytes() == blob and os.listdir(tmp_path) == ["o.fasta.gz"]
    assert es["out_bytes"] == len(text) == gs["in_bytes"] and gs["out_bytes"] == len(blob)


def test_gzip_a_window_that_keeps_nothing_and_nothing_at_all(engine):
    W = 65536
    drop = b">gone\n" + (b"ACGT" * 20 + b"\n") * 5
    table = Table([b"gone"], [400], [[(10, 20)]], [CHIMERIC])
    text = fillers(W + W // 2) + drop * (2 * W // len(drop) + 2) + fillers(W + 99)
    kept = text.replace(drop, b"")
    first = text.index(drop)
    assert first < 2 * W and first + 2 * W < text.rindex(drop)  # window 2 holds dropped records alone
    _gzip_is(engine, OP_FILTER, text, table, kept)
    _gzip_is(engine, OP_SCRUBB, text, table, restate(text, OP_SCRUBB, table)[0])
    assert _gzip_is(engine, OP_EXTRACT, fillers(3 * W + 5), Table(), b"") == _EOF_MEMBER


def test_gzip_an_output_longer_than_its_text(engine):
    """lines of 500 bases written again at 80 gain newlines: a window's output slot is sized by the scanned total"""
    W = 65536
    text = b"".join(record_of(5000 + i, b"wide%d" % i, width=500) for i in range(60))
    plain = restate(text, OP_FILTER, Table())[0]
    assert len(plain) > len(text) + 3000 and n_windows(text, W) >= 4
    _gzip_is(engine, OP_FILTER, text, Table(), plain)


# ---- 10: bounded memory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "gzip"])
def test_the_device_holds_a_ring_not_the_text(form):
    """the same records in 8 and in 64 windows: what the editor holds behind the edit does not grow with the text.  The bound:
    two text slots of 2 W, two output slots of a window's output (at most 2 W here), 32 bytes a line for at most 2 W / 81
    lines, and the tables per record, per tile and of the reads in the slack (gzip: the encoder's slots, by the batch)"""
    W = 65536
    rec = filler(1019)
    run = (lambda e, text: _gz(e, OP_FILTER, text, Table())) if form == "gzip" else (lambda e, text: _edit(e, OP_FILTER, text, Table()))
    with yacrd_amd.Engine(device_id=0) as e:
        e.debug_seq_window(W)
        run(e, rec * 200)
        e.trim()
        start = live_bytes()[0]
        held = {}
        for n_win in (8, 64):
            text = rec * (n_win * W // len(rec))
            out = run(e, text)
            assert (gzip.decompress(out) if form == "gzip" else out) == text
            w = e.seq_windows()
            assert w["windows"] == n_win
            held[n_win] = live_bytes()[0]
            print("held behind %d windows: %d bytes (ring %d + %d)" % (n_win, held[n_win] - start, w["text_ring_bytes"], w["out_ring_bytes"]))
            assert held[n_win] - start < 9 * W + (4 << 20 if form == "gzip" else 1 << 20)
            assert w["text_ring_bytes"] + w["out_ring_bytes"] <= held[n_win] - start
            e.trim()
            assert live_bytes()[0] == start
        assert held[64] <= held[8]


# ---- 11: the file form and the CLI ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_threads", [1, 6])
def test_file_form(engine, tmp_path, n_threads):
    """windows of 8 MiB: two chunks of the mover each, read by one thread and by six; and windows of a tile"""
    table = window_table()
    block = window_text(table, 5, 1 << 20)
    src, out = tmp_path / "in.fasta", tmp_path / "out.fasta"
    names, lengths, bo, br, rt = table.arrays()
    for W, text in ((8 << 20, block * 20), (W_SMALL, block)):
        src.write_bytes(text)
        engine.debug_seq_window(W)
        for op in (OP_SCRUBB, OP_FILTER):
            want, n_in, n_out = restate(text, op, table)
            st = engine.edit_fasta(op, str(src), str(out), names, lengths, (bo, br, rt), n_threads=n_threads)
            assert out.read_bytes() == want, (W, op)
            assert (st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(want), n_in, n_out)
            assert _ran_as(engine, text, W)["windows"] >= 3
    assert sorted(os.listdir(tmp_path)) == ["in.fasta", "out.fasta"]


def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


def test_cli_in_windows_on_a_generated_file(tmp_path):
    """the command on a generated .fasta and a report of the generator's table: with the switch at 64 KiB the editor's line
    ends in windows=K, and the file is the one the whole-text run writes"""
    table = window_table()
    text = window_text(table, 9, 1 << 20)
    src, rep = tmp_path / "gen.fasta", tmp_path / "gen.yacrd"
    src.write_bytes(text)
    kinds = ("NotBad", "Chimeric", "NotCovered")
    rep.write_bytes(b"".join(b"%s\t%s\t%d\t%s\n" % (kinds[t].encode(), n, l, b";".join(b"%d,%d,%d" % (e - b, b, e) for b, e in r))
                             for n, l, r, t in zip(table.names, table.lengths, table.regions, table.types)))
    for op in ("scrubb", "filter"):
        a, b = tmp_path / ("win_" + op + ".fasta"), tmp_path / ("whole_" + op + ".fasta")
        p = _cli(["-i", rep, "-o", tmp_path / "r.yacrd", "-n", "0.8", op, "-i", src, "-o", a], YACRD_CLI_TIMING="1", YACRD_SEQ_WINDOW="65536")
        assert p.returncode == 0, p.stderr
        line = [l for l in p.stderr.splitlines() if l.startswith("[info] device fasta editor:")]
        assert len(line) == 1 and int(line[0].rsplit("windows=", 1)[1]) == (len(text) + 65535) // 65536 > 0, p.stderr
        q = _cli(["-i", rep, "-o", tmp_path / "r2.yacrd", "-n", "0.8", op, "-i", src, "-o", b], YACRD_CLI_TIMING="1", YACRD_SEQ_WINDOW=str(_NEVER))
        assert q.returncode == 0, q.stderr
        line = [l for l in q.stderr.splitlines() if l.startswith("[info] device fasta editor:")]
        assert len(line) == 1 and line[0].endswith("windows=0"), q.stderr
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 1000 and a.read_bytes() != text, op
