"""The FASTQ editor window by window (csrc/gpu_seq_edit.hip: run_windows): a text of more than one window is edited
in a bounded ring of buffers, and the bytes do not change.  The yardsticks are the restatement and the host loop
(tests/edit_fastq_cases.py, pinned on the CPU), the windows' own rule (tests/edit_fastq_window_cases.py) and engine.gzip of the
plain bytes — never the whole-text run.  Every test reads seq_windows()["windows"]: none passes on the whole-text route."""
import gzip
import os
import subprocess

import pytest

import yacrd_amd
from edit_fastq_cases import CHIMERIC, OPS, OP_EXTRACT, OP_FILTER, OP_SCRUBB, Table, fallback_cases, fuzz_cases, host_loop, restate
from edit_fastq_window_cases import (W_SMALL, filler, fillers, long_record_text, missing_line_texts, record_of, window_carries, window_cases,
                                     window_table, window_text, windows_take)
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
_BLOCK = 65280     # bytes of text per BGZF member (csrc/bgzf_sizes.h: kBlock)
_EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_NEVER = 2 ** 64 - 1


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
    return engine.edit_fastq_text(op, text, names, lengths, (bo, br, rt))


def _gz(engine, op, text, table, out_path=None):
    names, lengths, bo, br, rt = table.arrays()
    return engine.edit_fastq_gzip(op, text, names, lengths, (bo, br, rt), out_path=out_path)


def _n_windows(text, W):
    return (len(text) + W - 1) // W if len(text) > W else 0


def _ran_as(engine, text, W):
    """the last edit ran in the windows the rule gives, and carried what the restatement carries"""
    w = engine.seq_windows()
    assert w["windows"] == _n_windows(text, W), w
    if w["windows"]:
        assert w["max_carry"] == max(window_carries(text, W)) and w["text_ring_bytes"] >= 2 * (2 * W + 64)
    return w


# ---- 1: generated texts ---------------------------------------------------------------------------------------------------------
def test_generated_texts_all_four_ops(engine, cases, tmp_path):
    for tag, text, table in cases:
        assert windows_take(text, W_SMALL) is True and _n_windows(text, W_SMALL) >= 40
        for op in OPS:
            want, n_in, n_out = restate(text, op, table)
            engine.debug_seq_window(W_SMALL)
            assert _edit(engine, op, text, table) == want, (tag, op)
            _ran_as(engine, text, W_SMALL)
            st = engine.seq_edit_stats
            assert (st["text_bytes"], st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(text), len(want), n_in, n_out), (tag, op)
            if op == OP_SCRUBB:
                assert want == host_loop(str(tmp_path), op, text, table), tag
            engine.debug_seq_window(_NEVER)
            assert _edit(engine, op, text, table) == want and engine.seq_windows()["windows"] == 0, (tag, op)


# ---- 2: every byte of a cut record as the first byte of window 1 -----------------------------------------------------------------
_TARGET = b"@target of the cut\n" + b"ACGT" * 10 + b"\n+\n" + bytes(range(40, 80)) + b"\n"
_TARGET_AT = b"@target of the cut\n" + b"ACGT" * 10 + b"\n+\n" + b"@" + bytes(range(41, 80)) + b"\n"  # its quality line begins with '@'
_TARGET_TABLE = Table([b"target"], [40], [[(5, 10), (20, 21)]], [CHIMERIC])


@pytest.mark.parametrize("target", [_TARGET, _TARGET_AT], ids=["plain", "quality_at"])
def test_border_sweep(engine, target, tmp_path):
    """two windows; byte `before` of the cut record is the first new byte of window 1: every line of the record crosses the
    border, the header between name and description, the '+' line and the quality line's first byte ('@') among them"""
    W = W_SMALL
    assert target.index(b"+\n") == 60 and target[62:63] in (b"(", b"@")
    engine.debug_seq_window(W)
    wants = {}
    for before in range(len(target)):
        text = fillers(W - before) + target + fillers(W // 2)
        assert text[W - before:].startswith(target) and W < len(text) <= 2 * W
        for op in OPS:
            want = restate(text, op, _TARGET_TABLE)[0]
            assert _edit(engine, op, text, _TARGET_TABLE) == want, (before, op)
            assert engine.seq_windows()["windows"] == 2 and engine.seq_windows()["max_carry"] == max(window_carries(text, W))
            wants[op] = (text, want)
    text, want = wants[OP_SCRUBB]
    assert want == host_loop(str(tmp_path), OP_SCRUBB, text, _TARGET_TABLE) and b"@target_0_5 of the cut\nACGTA\n+\n" in want


# ---- 3: the carry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [W_SMALL - 5, W_SMALL + 15], ids=["from_W-5", "from_W+15"])
def test_carry_chain(engine, first):
    """records of W - 10 bytes back to back: every window completes one record (now and then two) and carries what it holds
    of the next — from W + 15 on, nearly a whole window"""
    W = W_SMALL
    text = fillers(first) + b"".join(record_of(W - 10, b"c%02d" % i) for i in range(12)) + filler(55)
    engine.debug_seq_window(W)
    for op in (OP_SCRUBB, OP_FILTER, OP_EXTRACT):
        assert _edit(engine, op, text, Table()) == restate(text, op, Table())[0]
        w = _ran_as(engine, text, W)
    assert w["max_carry"] > (W - 200 if first > W else 100)


@pytest.mark.parametrize("at", [0, W_SMALL + 1, 2 * W_SMALL - 1])
def test_a_record_of_exactly_a_window_is_taken(engine, at):
    """at offsets 0, 1 and W - 1 of a window (a text cannot begin a record at its byte 1: window 1's byte 1 it is)"""
    W = W_SMALL
    text = (fillers(at) if at else b"") + record_of(W, b"bg") + filler(33)
    assert windows_take(text, W) is True and text[at:].startswith(b"@bg\n")
    engine.debug_seq_window(W)
    table = Table([b"bg"], [(W - 8) // 2], [[(7, 9)]], [CHIMERIC])
    for op in OPS:
        assert _edit(engine, op, text, table) == restate(text, op, table)[0], op
        _ran_as(engine, text, W)


def test_a_record_of_two_windows_and_a_byte_falls_back(engine):
    W = W_SMALL
    engine.debug_seq_window(W)
    with pytest.raises(yacrd_amd.NeedsHostParser, match="a record longer than a window"):
        _edit(engine, OP_FILTER, long_record_text(W), Table())
    assert engine.seq_windows()["windows"] == 0
    engine.debug_seq_window(_NEVER)
    assert _edit(engine, OP_FILTER, long_record_text(W), Table()) == long_record_text(W)


def test_long_records_of_the_fuzz_set(engine):
    """mid* / long* at W = 256 KiB, digits7 at 4 MiB: their records (<= 200 200 and 2 400 261 bytes) fit a window"""
    n = in_windows = 0
    for tag, text, table in fuzz_cases():
        W = 4 << 20 if tag == "digits7" else 256 << 10 if tag.startswith(("mid", "long")) else 0
        if not W:
            continue
        assert windows_take(text, W) is True, tag
        engine.debug_seq_window(W)
        for op in OPS:
            assert _edit(engine, op, text, table) == restate(text, op, table)[0], (tag, op)
            w = _ran_as(engine, text, W)
        n, in_windows = n + 1, in_windows + (w["windows"] >= 2)
    assert n == 9 and in_windows >= 3  # (long0, long1 and digits7 at the least: a mid* text may be shorter than its window)


# ---- 4: causes found late -------------------------------------------------------------------------------------------------------
def _falls_back_everywhere(engine, tmp_path, op, text, table):
    d = tmp_path / "dev"
    d.mkdir(exist_ok=True)
    src, out = tmp_path / "in.fastq", d / "out.fastq"
    src.write_bytes(text)
    out.write_bytes(b"what was there")
    names, lengths, bo, br, rt = table.arrays()
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _edit(engine, op, text, table)
    assert engine.seq_windows()["windows"] == 0
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.edit_fastq(op, str(src), str(out), names, lengths, (bo, br, rt))
    assert os.listdir(d) == ["out.fastq"] and out.read_bytes() == b"what was there"
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _gz(engine, op, text, table, out_path=str(d / "out.fastq.gz"))
    with pytest.raises(yacrd_amd.NeedsHostParser):
        _gz(engine, op, text, table, out_path=str(out))
    assert os.listdir(d) == ["out.fastq"] and out.read_bytes() == b"what was there"


_FALLBACKS = fallback_cases()


@pytest.mark.parametrize("tag,ops,bad,table", _FALLBACKS, ids=[f[0] for f in _FALLBACKS])
def test_fallback_causes_behind_three_good_windows(engine, tmp_path, tag, ops, bad, table):
    W = W_SMALL
    good = window_text(window_table(), 7, 3 * W + 100)  # (reads the case's table does not hold: copied, or dropped by extract)
    engine.debug_seq_window(W)
    assert _edit(engine, ops[0], good, table) == restate(good, ops[0], table)[0] and engine.seq_windows()["windows"] == 4
    _falls_back_everywhere(engine, tmp_path, ops[0], good + bad, table)


def test_a_deleted_line_and_a_missing_last_newline(engine, cases, tmp_path):
    W = W_SMALL
    tag, text, table = cases[0]
    text = window_text(table, 11, 6 * W)
    engine.debug_seq_window(W)
    assert _edit(engine, OP_SCRUBB, text, table) == restate(text, OP_SCRUBB, table)[0] and engine.seq_windows()["windows"] >= 6
    for what, broken in missing_line_texts(text, W):
        assert windows_take(broken, W) is False, what
        _falls_back_everywhere(engine, tmp_path, OP_SCRUBB, broken, table)


# ---- 5: gzip out ----------------------------------------------------------------------------------------------------------------
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
    """everything is kept, so the output is the input: window k's last whole record ends a byte before, on and a byte behind
    a border of the 65 280-byte blocks, and the windows' ends drift against the blocks from there"""
    W = 65536
    end = (k + 1) * _BLOCK + d
    text = fillers(end) + fillers(5 * W + 777)
    assert k * W < end <= (k + 1) * W and window_carries(text, W)[k] == (k + 1) * W - end
    blob = _gzip_is(engine, OP_FILTER, text, Table(), text)
    es, gs = _gz(engine, OP_FILTER, text, Table(), out_path=str(tmp_path / "o.fastq.gz"))
    assert (tmp_path / "o.fastq.gz").read_bytes() == blob and os.listdir(tmp_path) == ["o.fastq.gz"]
    assert es["out_bytes"] == len(text) == gs["in_bytes"] and gs["out_bytes"] == len(blob)


def test_gzip_a_window_that_keeps_nothing_and_nothing_at_all(engine):
    W = 65536
    drop = b"@gone\n" + b"ACGT" * 100 + b"\n+\n" + b"!" * 400 + b"\n"
    table = Table([b"gone"], [400], [[(10, 20)]], [CHIMERIC])
    text = fillers(W + W // 2) + drop * (2 * W // len(drop) + 2) + fillers(W + 99)
    kept = text.replace(drop, b"")
    first = text.index(drop)
    assert first < 2 * W and first + 2 * W < text.rindex(drop)  # window 2 holds dropped records alone
    _gzip_is(engine, OP_FILTER, text, table, kept)
    _gzip_is(engine, OP_SCRUBB, text, table, restate(text, OP_SCRUBB, table)[0])
    assert _gzip_is(engine, OP_EXTRACT, fillers(3 * W + 5), Table(), b"") == _EOF_MEMBER


# ---- 6: bounded memory ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "gzip"])
def test_the_device_holds_a_ring_not_the_text(form):
    """the same records in 8 and in 64 windows: what the editor holds behind the edit does not grow with the text"""
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
            assert held[n_win] - start < 12 * W + (4 << 20 if form == "gzip" else 1 << 20)  # (gzip: the encoder's slots, by the batch and not by the text)
            assert w["text_ring_bytes"] + w["out_ring_bytes"] <= held[n_win] - start
            e.trim()
            assert live_bytes()[0] == start
        assert held[64] <= held[8]


# ---- 7: the file form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_threads", [1, 6])
def test_file_form(engine, tmp_path, n_threads):
    """windows of 8 MiB: two chunks of the mover each, read by one thread and by six; and windows of a tile"""
    table = window_table()
    block = window_text(table, 5, 1 << 20)
    src, out = tmp_path / "in.fastq", tmp_path / "out.fastq"
    names, lengths, bo, br, rt = table.arrays()
    for W, text in ((8 << 20, block * 20), (W_SMALL, block)):
        src.write_bytes(text)
        engine.debug_seq_window(W)
        for op in (OP_SCRUBB, OP_FILTER):
            want, n_in, n_out = restate(text, op, table)
            st = engine.edit_fastq(op, str(src), str(out), names, lengths, (bo, br, rt), n_threads=n_threads)
            assert out.read_bytes() == want, (W, op)
            assert (st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(want), n_in, n_out)
            assert _ran_as(engine, text, W)["windows"] >= 3
    assert sorted(os.listdir(tmp_path)) == ["in.fastq", "out.fastq"]


# ---- 8: the CLI -----------------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


@pytest.mark.parametrize("form", ["plain", "gzip1"])
def test_cli_in_windows_on_the_fixture(golden_dir, tmp_path, form):
    text = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read()
    assert len(text) == 1059085
    ext = ".fastq" if form == "plain" else ".fastq.gz"
    src = tmp_path / ("reads" + ext)
    src.write_bytes(text if form == "plain" else gzip.compress(text, 1))
    rep = os.path.join(golden_dir, "truth.yacrd")
    for op in ("scrubb", "filter"):
        a, b = tmp_path / ("dev_" + op + ext), tmp_path / ("host_" + op + ext)
        p = _cli(["-i", rep, "-o", tmp_path / "r.yacrd", "-n", "0.8", op, "-i", src, "-o", a], YACRD_CLI_TIMING="1", YACRD_SEQ_WINDOW="65536")
        assert p.returncode == 0, p.stderr
        line = [l for l in p.stderr.splitlines() if l.startswith("[info] device fastq editor:")]
        assert len(line) == 1 and int(line[0].rsplit("windows=", 1)[1]) == (len(text) + 65535) // 65536, p.stderr
        q = _cli(["-i", rep, "-o", tmp_path / "r2.yacrd", "-n", "0.8", op, "-i", src, "-o", b], YACRD_CLI_TIMING="1", YACRD_NO_DEVICE_EDITOR="1")
        assert q.returncode == 0 and "[info] device fastq editor" not in q.stderr, q.stderr
        truth = gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % op), "rb").read()
        got, want = a.read_bytes(), b.read_bytes()
        if form != "plain":
            assert got[:2] == b"\x1f\x8b"
            got, want = gzip.decompress(got), gzip.decompress(want)
        assert got == want == truth, op
