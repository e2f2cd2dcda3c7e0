"""The overlap editor window by window (csrc/gpu_edit.hip: windows_loop): a plain text of more than one window is
edited in a ring of buffers whose size does not depend on the text, and the bytes are those of the whole-text run.  The
yardsticks are the restatement of edit_overlaps_cases, the host loop and engine.gzip of the plain bytes — never the whole-text
run.  Every test reads edit_windows()["windows"]: none passes on the whole-text route."""
import gzip
import os
import shutil
import subprocess

import pytest

import edit_overlaps_window_cases as wc
import yacrd_amd
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, TILE, host_loop, restate
from edit_overlaps_window_cases import NAMES, TABLE, TYPES, bad, fill, good, n_windows, window_reaches
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
W = wc.W_TEST
C = wc.chunk_of(W)
_NEVER = 2 ** 64 - 1
OPS = (OP_FILTER, OP_EXTRACT)
GZ_BLOCK = 65280


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e
        e.debug_edit_window(0)


def _fmt(m4):
    return 2 if m4 else 1


def _windowed(engine, op, text, m4, names=NAMES, types=TYPES, table=TABLE, w=W):
    """the edit in windows of `w` against the restatement: bytes, stats, the windows and the farthest reach -> the kept bytes"""
    engine.debug_edit_window(w)
    got = engine.edit_overlaps_text(op, text, names, types, _fmt(m4))
    want, n_lines, n_kept = restate(text, op, table, m4)
    assert got == want, (op, m4, len(text))
    st, ew = engine.edit_stats, engine.edit_windows()
    assert (st["n_lines"], st["n_kept"], st["text_bytes"], st["kept_bytes"]) == (n_lines, n_kept, len(text), len(want))
    assert ew["windows"] == n_windows(text, w) > 1 and ew["max_reach"] == max(window_reaches(text, w))
    return got


# ---- 1. generated texts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_generated_texts(engine, tmp_path, m4):
    text, names, types = wc.generated(20250607 + m4, m4, W)
    table = dict(zip(names, types))
    assert n_windows(text, W) == 40
    for op in OPS:
        got = _windowed(engine, op, text, m4, names, types, table)
        if op == OP_FILTER:
            assert got == host_loop(str(tmp_path), op, text, names, types, ".m4" if m4 else ".paf")
        engine.debug_edit_window(_NEVER)
        assert engine.edit_overlaps_text(op, text, names, types, _fmt(m4)) == got and engine.edit_windows()["windows"] == 0


# ---- 2. border sweep ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_kept", [True, False], ids=["kept", "dropped"])
@pytest.mark.parametrize("op", OPS, ids=["filter", "extract"])
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_border_sweep(engine, m4, op, want_kept):
    """every byte of a line, in turn, is the first byte of window 1; its neighbours have the opposite verdict"""
    cases = wc.border_sweep(m4, W, want_kept, op)
    assert len(cases) == 101
    for cut, text in cases:
        got = _windowed(engine, op, text, m4)
        assert (text[W - cut:W - cut + 101] in got) == want_kept, cut
        assert engine.edit_windows()["windows"] == 2 and engine.edit_windows()["max_reach"] == (101 - cut if cut else 0)


# ---- 3. a window without a line start ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_a_window_without_a_line_start(engine, m4):
    for target in (good, bad):
        text = wc.no_start_window(m4, W, target)
        for op in OPS:
            got = _windowed(engine, op, text, m4)
            assert (text[2 * W - 1:3 * W] in got) == ((target is good) == (op == OP_FILTER))
            assert engine.edit_windows()["windows"] == 4 and engine.edit_windows()["max_reach"] == W


# ---- 4. look-ahead edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_look_ahead_edges(engine, tmp_path, m4):
    for maker in (good, bad):
        for reach in (C - 1, C):
            text = wc.reaching(m4, W, reach, maker)
            assert wc.windows_take(text, W)
            for op in OPS:
                _windowed(engine, op, text, m4)
                assert engine.edit_windows()["max_reach"] == reach
    # one byte more: the text is the host loop's, nothing is written and nothing is left beside the output
    text = wc.reaching(m4, W, C + 1, bad)
    assert wc.windows_take(text, W) is False
    engine.debug_edit_window(W)
    src, d = tmp_path / ("in" + (".m4" if m4 else ".paf")), tmp_path / "out"
    d.mkdir()
    src.write_bytes(text)
    for op in OPS:
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps_text(op, text, NAMES, TYPES, _fmt(m4))
        assert engine.edit_windows()["windows"] == 0
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps(op, str(src), str(d / "o.txt"), NAMES, TYPES)
        assert engine.edit_windows()["windows"] == 0 and os.listdir(d) == []
    # ... and the file form takes what the memory form takes, with the same report
    text = wc.reaching(m4, W, C, bad)
    src.write_bytes(text)
    st = engine.edit_overlaps(OP_EXTRACT, str(src), str(d / "o.txt"), NAMES, TYPES)
    assert (d / "o.txt").read_bytes() == restate(text, OP_EXTRACT, TABLE, m4)[0] and st["kept_bytes"] == (d / "o.txt").stat().st_size
    assert engine.edit_windows()["windows"] == n_windows(text, W) and engine.edit_windows()["max_reach"] == C and os.listdir(d) == ["o.txt"]


@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_last_lines_empty_lines_and_whole_windows(engine, m4):
    for maker in (good, bad):
        other = bad if maker is good else good
        # a last line without its newline: in the last window; reaching into it (to its last byte but one, to its last byte)
        texts = [fill(m4, 2 * W + 100, other) + maker(m4, 200),
                 wc.reaching(m4, W, 300, maker, newline=False, behind=False),
                 wc.reaching(m4, W, C - 1, maker, newline=False, behind=False),
                 wc.reaching(m4, W, C, maker, newline=False, behind=False)]
        # empty lines across a border: the border between two newlines, in front of the first, behind the last
        for lead in (W - 2, W - 1, W):
            texts.append(fill(m4, lead, maker) + b"\n\n\n" + fill(m4, W, other))
        # a text of exactly k W and k W +- 1 bytes, with and without its last newline (k W without: the newline it gets
        # opens a tile of its own)
        for size in (2 * W - 1, 2 * W, 2 * W + 1, 3 * W):
            whole = fill(m4, size - 300, other) + maker(m4, 299) + b"\n"
            texts += [whole, whole[:-1] + b"7", whole[:-1]]
        for text in texts:
            for op in OPS:
                _windowed(engine, op, text, m4)
    text = wc.reaching(m4, W, C + 1, bad, newline=False, behind=False)
    engine.debug_edit_window(W)
    with pytest.raises(yacrd_amd.NeedsHostParser):
        engine.edit_overlaps_text(OP_EXTRACT, text, NAMES, TYPES, _fmt(m4))
    assert engine.edit_windows()["windows"] == 0


# ---- 5. gzip out -------------------------------------------------------------------------------------------------------
def _gzip_windowed(engine, op, text, m4, w, names=NAMES, types=TYPES, table=TABLE):
    engine.debug_edit_window(w)
    got = engine.edit_overlaps_gzip(op, text, names, types, _fmt(m4))
    want = restate(text, op, table, m4)[0]
    assert engine.edit_windows()["windows"] == n_windows(text, w) > 1
    assert got == engine.gzip(want), (op, m4, w, len(text), len(want))
    assert gzip.decompress(got) == want and engine.gzip_stats["in_bytes"] == len(want)
    return want


@pytest.mark.parametrize("w", [TILE, 2 * TILE, 3 * TILE], ids=["32K", "64K", "96K"])
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_gzip_out_is_the_stream_of_the_kept_bytes(engine, m4, w):
    """blocks of 65 280 bytes counted from byte 0 of the kept stream: their borders fall before, on and behind window borders"""
    text, names, types = wc.generated(20250608 + m4, m4, TILE, windows=24)
    table = dict(zip(names, types))
    for op in OPS:
        _gzip_windowed(engine, op, text, m4, w, names, types, table)
    # everything kept: the stream's blocks are the text's own, so a block ends 255 k bytes in front of window border 2 k
    everything = fill(m4, 12 * TILE + 5, good)
    assert len(_gzip_windowed(engine, OP_FILTER, everything, m4, w)) == len(everything)
    # kept bytes that end exactly on a block's border, one byte before and one behind it
    for d in (-1, 0, 1):
        text = fill(m4, 2 * GZ_BLOCK + d, good) + fill(m4, 2 * TILE, bad)
        assert len(_gzip_windowed(engine, OP_FILTER, text, m4, w)) == 2 * GZ_BLOCK + d


@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_gzip_out_windows_that_keep_nothing(engine, tmp_path, m4):
    # a tail of 1000 bytes is handed through five windows that keep nothing, then encoded with what the last ones keep
    text = fill(m4, 1000, good) + fill(m4, 6 * W, bad) + fill(m4, W + 4000, good)
    assert len(_gzip_windowed(engine, OP_FILTER, text, m4, W)) == W + 5000
    assert len(_gzip_windowed(engine, OP_EXTRACT, text, m4, W)) == 6 * W
    # ... and is all there is
    assert len(_gzip_windowed(engine, OP_FILTER, fill(m4, 1000, good) + fill(m4, 6 * W, bad), m4, W)) == 1000
    # nothing kept at all: the EOF member alone
    nothing = fill(m4, 5 * W + 17, bad)
    assert _gzip_windowed(engine, OP_FILTER, nothing, m4, W) == b"" and len(engine.gzip(b"")) == 28
    # into a file; a fallback found in a late window (members of earlier windows have been written by then) leaves none
    d = tmp_path / "out"
    d.mkdir()
    engine.debug_edit_window(W)
    st, gs = engine.edit_overlaps_gzip(OP_EXTRACT, text, NAMES, TYPES, _fmt(m4), out_path=str(d / "o.gz"))
    assert (d / "o.gz").read_bytes() == engine.gzip(restate(text, OP_EXTRACT, TABLE, m4)[0]) and engine.edit_windows()["windows"] == n_windows(text, W)
    os.remove(d / "o.gz")
    late = fill(m4, 9 * W - 50, good) + bad(m4, 50 + C) + b"\n" + fill(m4, 1000, good)
    assert wc.windows_take(late, W) is False and window_reaches(late, W)[8] == C + 1
    for out_path in (str(d / "late.gz"), None):
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps_gzip(OP_FILTER, late, NAMES, TYPES, _fmt(m4), out_path=out_path)
        assert engine.edit_windows()["windows"] == 0 and os.listdir(d) == []


# ---- 6. bounded footprint ----------------------------------------------------------------------------------------------
def test_the_ring_does_not_grow_with_the_text():
    before = live_bytes()
    with yacrd_amd.Engine(device_id=0) as e:
        e.debug_edit_window(W)
        rings = []
        for windows in (40, 80):
            text = fill(False, windows * W - 123, good)[:-1]
            assert e.edit_overlaps_text(OP_FILTER, text, NAMES, TYPES, 1) == text + b"\n"
            assert gzip.decompress(e.edit_overlaps_gzip(OP_FILTER, text, NAMES, TYPES, 1)) == text + b"\n"
            ew = e.edit_windows()
            assert ew["windows"] == windows
            rings.append((ew["text_ring_bytes"], ew["out_ring_bytes"]))
        assert rings[0] == rings[1]
        assert 2 * W < rings[0][0] <= 2 * (W + C + 80) * 1.125 and 2 * W < rings[0][1] <= 2 * (W + GZ_BLOCK + 64) * 1.125
        text = fill(False, 80 * W, bad)
        stream = e.gzip(text)  # (the yardstick first: its buffers are the text's size and go with the trim)
        e.trim()
        warm = live_bytes()  # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers)
        assert e.edit_overlaps_text(OP_EXTRACT, text, NAMES, TYPES, 1) == text and e.edit_windows()["windows"] == 80
        assert e.edit_overlaps_gzip(OP_EXTRACT, text, NAMES, TYPES, 1) == stream
        held = live_bytes()
        assert warm[0] + sum(rings[0]) < held[0] < warm[0] + len(text)  # (the ring and the tables: less than the text)
        e.trim()
        assert live_bytes() == warm
    assert live_bytes() == before


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))


def _editor_line(p, stream):
    hit = [l for l in stream.splitlines() if l.startswith("[info] device editor")]
    assert p.returncode == 0 and len(hit) == 1, p.stderr
    return hit[0]


@pytest.mark.parametrize("op", ["filter", "extract"])
@pytest.mark.parametrize("form", ["plain", "gzip"])
def test_cli_with_the_window_set(golden_dir, tmp_path, op, form):
    ext = ".paf" if form == "plain" else ".paf.gz"
    src = tmp_path / ("copy" + ext)  # (not the detection's own file: the text is moved, not taken from the parser's mirror)
    text = open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    src.write_bytes(text if form == "plain" else gzip.compress(text, 1))  # (one plain gzip member: inflated on the host, edited as text)
    paf = tmp_path / "reads.paf"
    shutil.copy(os.path.join(golden_dir, "reads.paf"), paf)
    a, b = tmp_path / ("win" + ext), tmp_path / ("whole" + ext)
    args = ["-i", paf, "-o", tmp_path / "r.yacrd", "-c", "4", "-n", "0.4", op, "-i", src, "-o"]
    p = _cli(args + [a], YACRD_CLI_TIMING="1", YACRD_EDIT_WINDOW=str(W))
    q = _cli(args + [b], YACRD_CLI_TIMING="1")
    lp, lq = (_editor_line(x, x.stderr if form == "plain" else x.stdout) for x in (p, q))
    k = int(lp.rsplit(" windows=", 1)[1])
    assert k == n_windows(text, W) > 1 and lq.endswith(" windows=0"), (lp, lq)
    assert a.read_bytes() == b.read_bytes() and a.stat().st_size > 0
    inflated = a.read_bytes() if form == "plain" else gzip.decompress(a.read_bytes())
    assert 0 < len(inflated) < len(text) and inflated.count(b"\n") == (1286 - 448 if op == "filter" else 448)
