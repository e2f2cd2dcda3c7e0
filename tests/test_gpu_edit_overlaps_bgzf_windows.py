"""The overlap editor window by window over a BGZF text (csrc/gpu_edit.hip: bgzf_windows_loop): the windows are
the member table's cuts that hold text — they end where a member ends, anywhere inside a tile —, each inflated into its text
slot out of one compressed slot, edited by the same kernels, and the bytes are those of the plain text's edit.  The yardsticks
are the restatement of edit_overlaps_cases, the host loop and Engine.gzip of the plain kept bytes — never the whole-text
device run.  Every test reads edit_windows()["windows"]: none passes where the BGZF forms run whole."""
import gzip
import os
import subprocess

import pytest

import edit_overlaps_bgzf_window_cases as bc
import inflate_cases as ic
import yacrd_amd
from deflate_cases import EOF_MEMBER
from edit_bgzf_window_cases import cuts_of
from edit_overlaps_bgzf_window_cases import NAMES, TABLE, TYPES, bad, fill, good
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, TILE, host_loop, restate
from test_edit_overlaps_bgzf_window_cases import GENERATED, OFFSETS, generated_case
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
W = bc.W_TEST
C = bc.chunk_of(W)
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


def _windowed(engine, op, blob, text, m4, names=NAMES, types=TYPES, table=TABLE, w=W, gz=False):
    """the edit of `blob` in windows of `w` against the restatement: bytes, stats, the windows and the farthest reach"""
    wins = bc.windows_of(cuts_of(blob, bc.bgzf_window(w)), bc.bgzf_window(w))
    assert bc.refused(text, wins) == []
    engine.debug_edit_window(w)
    got = engine.edit_overlaps_bgzf(op, blob, names, types, _fmt(m4), gzip_out=gz)
    want, n_lines, n_kept = restate(text, op, table, m4)
    if gz:
        assert got == engine.gzip(want) and gzip.decompress(got) == want and engine.gzip_stats["in_bytes"] == len(want), (op, m4, len(text))
    else:
        assert got == want, (op, m4, len(text))
    st, ew, us = engine.edit_stats, engine.edit_windows(), engine.inflate_stats
    assert (st["n_lines"], st["n_kept"], st["text_bytes"], st["kept_bytes"]) == (n_lines, n_kept, len(text), len(want))
    assert (us["in_bytes"], us["out_bytes"]) == (len(blob), len(text))
    assert ew["windows"] == len(wins) > 1 and ew["max_reach"] == max(bc.window_reaches(text, wins))
    return want


# ---- 1. generated texts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,m4,stream", GENERATED, ids=["%s-%s" % ("m4" if m else "paf", s) for _, m, s in GENERATED])
def test_generated_texts(engine, tmp_path, seed, m4, stream):
    text, names, types, blob = generated_case(seed, m4, stream)
    table = dict(zip(names, types))
    for op in OPS:
        for gz in (False, True):
            got = _windowed(engine, op, blob, text, m4, names, types, table, gz=gz)
        if op == OP_FILTER:
            assert got == host_loop(str(tmp_path), op, text, names, types, ".m4" if m4 else ".paf")
        engine.debug_edit_window(_NEVER)
        assert engine.edit_overlaps_bgzf(op, blob, names, types, _fmt(m4), gzip_out=False) == got and engine.edit_windows()["windows"] == 0
    # into a file, and at windows of 96 and 128 KiB
    out = tmp_path / "o.gz"
    engine.debug_edit_window(W)
    engine.edit_overlaps_bgzf(OP_EXTRACT, blob, names, types, _fmt(m4), out_path=str(out))
    assert out.read_bytes() == engine.gzip(restate(text, OP_EXTRACT, table, m4)[0]) and engine.edit_windows()["windows"] > 1
    for w in (W + TILE, 2 * W):
        _windowed(engine, OP_FILTER, blob, text, m4, names, types, table, w=w, gz=True)
        _windowed(engine, OP_EXTRACT, blob, text, m4, names, types, table, w=w)


# ---- 2. a window that ends inside a tile -------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("want_kept", [True, False], ids=["kept", "dropped"])
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_a_window_ends_inside_a_tile(engine, m4, want_kept, off):
    """window 0 ends at offset `off` of a tile — the 64-bit mask words, the 128-byte granule of a thread, the tile's last byte —
    and every byte of a 101-byte line is in turn the first byte of window 1; its neighbours have the opposite verdict"""
    for op in OPS:
        for cut, text, T in bc.border_sweep(m4, off, want_kept, op):
            blob = bc.with_windows(text, [T, bc.SWEEP_NEXT])
            got = _windowed(engine, op, blob, text, m4)
            assert (text[T - cut:T - cut + 101] in got) == want_kept, cut
            assert engine.edit_windows()["windows"] == 2 and engine.edit_windows()["max_reach"] == (101 - cut if cut else 0)


# ---- 3. windows and look-ahead edges -----------------------------------------------------------------------------------------
SHORT = [60000, 10000, 60000]  # a short window between two long ones: ahead_0 = 10 000 < C


@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_a_window_without_a_line_start(engine, m4):
    """window 1's last byte is the newline of a line begun in window 0: its 10 000 bytes are all that line's"""
    for target in (good, bad):
        other = bad if target is good else good
        text = fill(m4, 59000, other) + target(m4, 1000 + 10000 - 1) + b"\n" + fill(m4, 60000, other)
        assert text[69999:70000] == b"\n" and b"\n" not in text[59000:69999]
        blob = bc.with_windows(text, SHORT)
        for op in OPS:
            got = _windowed(engine, op, blob, text, m4)
            assert (text[59000:70000] in got) == ((target is good) == (op == OP_FILTER))
            assert engine.edit_windows()["windows"] == 3 and engine.edit_windows()["max_reach"] == 10000
        _windowed(engine, OP_FILTER, blob, text, m4, gz=True)


@pytest.mark.parametrize("lens,T,ahead", [([W, W, 1000], W, C), (SHORT, 60000, 10000)], ids=["ahead=C", "short-next-window"])
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_look_ahead_edges(engine, tmp_path, m4, lens, T, ahead):
    for maker in (good, bad):
        for reach in (ahead - 1, ahead):
            text = bc.reaching(m4, T, reach, maker, behind=sum(lens) - T - reach)
            blob = bc.with_windows(text, lens)
            for op in OPS:
                _windowed(engine, op, blob, text, m4)
                assert engine.edit_windows()["max_reach"] == reach
    # one byte more: the text is the host loop's, nothing is written, no file is left, the engine is usable
    text = bc.reaching(m4, T, ahead + 1, bad, behind=sum(lens) - T - ahead - 1)
    blob = bc.with_windows(text, lens)
    assert bc.windows_take(text, blob, W) is False
    d = tmp_path / "out"
    d.mkdir()
    engine.debug_edit_window(W)
    for op in OPS:
        for gz in (False, True):
            with pytest.raises(yacrd_amd.NeedsHostParser):
                engine.edit_overlaps_bgzf(op, blob, NAMES, TYPES, _fmt(m4), gzip_out=gz)
            assert engine.edit_windows()["windows"] == 0
            with pytest.raises(yacrd_amd.NeedsHostParser):
                engine.edit_overlaps_bgzf(op, blob, NAMES, TYPES, _fmt(m4), out_path=str(d / "o"), gzip_out=gz)
            assert engine.edit_windows()["windows"] == 0 and os.listdir(d) == []
    engine.debug_edit_window(_NEVER)
    assert engine.edit_overlaps_bgzf(OP_EXTRACT, blob, NAMES, TYPES, _fmt(m4), gzip_out=False) == restate(text, OP_EXTRACT, TABLE, m4)[0]


@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_last_lines_and_empty_lines(engine, m4):
    for maker in (good, bad):
        other = bad if maker is good else good
        cases = []
        # a last line without its newline: in the last window; begun in window 0, in a last window that lies wholly inside the look-ahead
        cases.append((fill(m4, 60000 + 9000, other) + maker(m4, 1000), [60000, 10000]))
        cases.append((bc.reaching(m4, 60000, 10000, maker, newline=False, behind=0), [60000, 10000]))
        cases.append((bc.reaching(m4, 60000, 9999, maker, newline=False, behind=0), [60000, 9999]))
        # empty lines across a border: the border between two newlines, in front of the first, behind the last
        for lead in (59998, 59999, 60000):
            text = fill(m4, lead, maker) + b"\n\n\n"
            cases.append((text + fill(m4, 120000 - len(text), other), [60000, 60000]))
        # a text that ends with its window's tile, with and without its last newline (without: the newline it gets opens a tile)
        whole = fill(m4, 60000 + TILE - 300, other) + maker(m4, 299) + b"\n"
        cases += [(whole, [60000, TILE]), (whole[:-1] + b"7", [60000, TILE]), (whole[:-1], [60000, TILE - 1])]
        for text, lens in cases:
            blob = bc.with_windows(text, lens)
            for op in OPS:
                _windowed(engine, op, blob, text, m4)
            _windowed(engine, OP_FILTER if maker is good else OP_EXTRACT, blob, text, m4, gz=True)


# ---- 4. members --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_empty_members_a_trailing_eof_cut_and_no_eof(engine, m4):
    text = fill(m4, 50000, good) + fill(m4, 40000, bad) + fill(m4, 40000, good)
    for eof, empties in ((True, (1,)), (True, (0, 1, 2)), (False, ()), (False, (2,))):
        blob = bc.with_windows(text, SHORT[:1] + [10000, 60000], eof=eof, empties=empties)
        for op in OPS:
            _windowed(engine, op, blob, text, m4)
    # more than a window of empty members mid-stream: cuts without text between two windows
    front, back = fill(m4, 60000, good), fill(m4, 60000, bad)
    blob = ic.stored_member(front) + EOF_MEMBER * 5000 + ic.stored_member(back) + EOF_MEMBER
    cuts = cuts_of(blob, W)
    assert len(cuts) >= 4 and len(bc.windows_of(cuts, W)) == 2 and any(c[5] == c[4] for c in cuts[1:-1])
    for op in OPS:
        _windowed(engine, op, blob, front + back, m4)
    # the EOF member in a cut of its own behind the last window (stored frames of 65 536 bytes fill the stream cap)
    text = fill(m4, 3 * 65505, good)[:-1]
    blob = bc.with_windows(text, [65505, 65505, 65504])
    cuts = cuts_of(blob, W)
    assert cuts[-1][5] == cuts[-1][4] and len(bc.windows_of(cuts, W)) == 3
    assert _windowed(engine, OP_FILTER, blob, text, m4, gz=True) == text + b"\n"


# ---- 5. refusals found in a late window --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_refusals_in_window_8(engine, tmp_path, m4):
    """a member the decoder does not take (a damaged CRC) and a text the editor does not take (a '"', a CR), each in window 8:
    earlier windows' output has left by then — nothing is returned, no file is left, the next edit is correct"""
    lens = [60000] * 12
    text = fill(m4, sum(lens), good)
    blob = bc.with_windows(text, lens)
    at = [c[3] for c in cuts_of(blob, W)][8]  # the end of window 8's frame: its CRC32 lies 8 bytes in front of it
    crc = bytearray(blob)
    crc[at - 8] ^= 0x55
    damaged = [bytes(crc)]
    for ch in (b'"', b"\r"):
        t = bytearray(text)
        t[8 * 60000 + 30000] = ch[0]
        damaged.append(bc.with_windows(bytes(t), lens))
    d = tmp_path / "out"
    d.mkdir()
    for blob_bad in damaged:
        engine.debug_edit_window(W)
        for gz in (False, True):
            with pytest.raises(yacrd_amd.NeedsHostParser):
                engine.edit_overlaps_bgzf(OP_FILTER, blob_bad, NAMES, TYPES, _fmt(m4), gzip_out=gz)
            assert engine.edit_windows()["windows"] == 0
            with pytest.raises(yacrd_amd.NeedsHostParser):
                engine.edit_overlaps_bgzf(OP_FILTER, blob_bad, NAMES, TYPES, _fmt(m4), out_path=str(d / "o"), gzip_out=gz)
            assert engine.edit_windows()["windows"] == 0 and os.listdir(d) == []
        assert _windowed(engine, OP_FILTER, blob, text, m4) == text


# ---- 6. gzip out -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [W, W + TILE, 2 * W], ids=["64K", "96K", "128K"])
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_gzip_out_is_the_stream_of_the_kept_bytes(engine, m4, w):
    # whole windows that keep nothing: a tail of 1000 bytes is handed through them, then encoded with what the last ones keep
    text = fill(m4, 1000, good) + fill(m4, 6 * W, bad) + fill(m4, W + 4000, good)
    blob = bc.own_stream(text)
    assert len(_windowed(engine, OP_FILTER, blob, text, m4, w=w, gz=True)) == W + 5000
    assert len(_windowed(engine, OP_EXTRACT, blob, text, m4, w=w, gz=True)) == 6 * W
    # kept bytes that end exactly on a block's border, one byte before and one behind it
    for d in (-1, 0, 1):
        text = fill(m4, 2 * GZ_BLOCK + d, good) + fill(m4, 3 * W, bad)
        assert len(_windowed(engine, OP_FILTER, bc.own_stream(text, "stored"), text, m4, w=w, gz=True)) == 2 * GZ_BLOCK + d
    # nothing kept at all: the EOF member alone
    nothing = fill(m4, 5 * W + 17, bad)
    assert _windowed(engine, OP_FILTER, bc.own_stream(nothing, "level6"), nothing, m4, w=w, gz=True) == b"" and len(engine.gzip(b"")) == 28


# ---- 7. bounded footprint ----------------------------------------------------------------------------------------------------
def test_the_ring_does_not_grow_with_the_text():
    before = live_bytes()
    with yacrd_amd.Engine(device_id=0) as e:
        e.debug_edit_window(W)
        rings = []
        for windows in (20, 40):
            text = fill(False, windows * 65280 - 123, good)[:-1]
            blob = bc.own_stream(text)
            assert e.edit_overlaps_bgzf(OP_FILTER, blob, NAMES, TYPES, 1, gzip_out=False) == text + b"\n"
            assert gzip.decompress(e.edit_overlaps_bgzf(OP_FILTER, blob, NAMES, TYPES, 1)) == text + b"\n"
            ew = e.edit_windows()
            assert ew["windows"] == windows
            rings.append((ew["text_ring_bytes"], ew["out_ring_bytes"]))
        assert rings[0] == rings[1]
        # two text slots, the compressed slot and the member slice; two output slots
        assert 3 * W < rings[0][0] <= (2 * (W + C + 80) + W + 64 + 4096) * 1.125 and 2 * W < rings[0][1] <= 2 * (W + GZ_BLOCK + 64) * 1.125
        text = fill(False, 40 * 65280, bad)
        blob = bc.own_stream(text)
        e.trim()
        warm = live_bytes()  # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers)
        assert e.edit_overlaps_bgzf(OP_EXTRACT, blob, NAMES, TYPES, 1, gzip_out=False) == text and e.edit_windows()["windows"] == 40
        held = live_bytes()
        assert warm[0] + rings[0][0] < held[0] < warm[0] + len(text)  # (the ring and the tables: less than the text)
        e.trim()
        assert live_bytes() == warm
    assert live_bytes() == before


# ---- 8. the CLI --------------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    base = {k: v for k, v in os.environ.items() if k not in ("YACRD_DEVICE_INFLATE", "YACRD_NO_DEVICE_INFLATE", "YACRD_EDIT_WINDOW")}
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(base, **env))
    assert p.returncode == 0, p.stderr
    return p


@pytest.mark.parametrize("op", ["filter", "extract"])
def test_cli_on_a_bgzf_copy(golden_dir, tmp_path, op):
    text = open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    blob = ic.bgzf_of(text, level=6)
    x, copy = tmp_path / "x.paf.gz", tmp_path / "copy.paf.gz"  # (a copy, another inode: the editor's own _bgzf_ form)
    x.write_bytes(blob), copy.write_bytes(blob)

    def run(tag, **env):
        out = tmp_path / (tag + ".paf.gz")
        p = _cli(["-i", x, "-o", tmp_path / (tag + ".yacrd"), "-c", "4", "-n", "0.4", op, "-i", copy, "-o", out], YACRD_CLI_TIMING="1", **env)
        hit = [l for l in p.stdout.splitlines() if l.startswith("[info] device editor")]
        return hit, out.read_bytes()

    lp, got = run("win", YACRD_EDIT_WINDOW=str(W))
    lq, whole = run("whole", YACRD_EDIT_WINDOW=str(_NEVER))
    lh, host_out = run("host", YACRD_NO_DEVICE_EDITOR="1")
    assert len(lp) == len(lq) == 1 and lh == []
    assert "resident=0 device_inflate=1" in lp[0] and lq[0].endswith(" windows=0")
    assert int(lp[0].rsplit(" windows=", 1)[1]) == len(bc.windows_of(cuts_of(blob, W), W)) > 1, lp
    assert got == whole and gzip.decompress(got) == gzip.decompress(host_out)
    assert gzip.decompress(got).count(b"\n") == (1286 - 448 if op == "filter" else 448)
