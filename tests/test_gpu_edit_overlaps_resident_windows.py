"""The overlap editor window by window over a text that is already in HBM (csrc/gpu_edit.hip: windows_loop from the mirror;
DESIGN 7o): the resident forms (Engine.edit_overlaps_resident, after ingest_text / ingest_bgzf / ingest_paf) and the edit of
the very file the engine last ingested (Engine.edit_overlaps: the parser's mirror) take the route of 7n — no text slot is
held, window k is the mirror's bytes from k W on, the output goes through the ring of two slots.  The yardsticks are the
restatement of edit_overlaps_cases, the host loop and Engine.gzip of the plain kept bytes — never the whole-text device run.
Every test reads edit_windows()["windows"]: none passes where these forms run whole."""
import gzip
import os
import shutil
import subprocess

import pytest

import edit_overlaps_resident_window_cases as rc
import inflate_cases as ic
import yacrd_amd
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, host_loop, restate
from edit_overlaps_resident_window_cases import NAMES, TABLE, TYPES, bad, fill, good, n_windows, window_reaches
from yacrd_amd.engine import live_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
W = rc.W_TEST
C = rc.chunk_of(W)
_NEVER = 2 ** 64 - 1
OPS = (OP_FILTER, OP_EXTRACT)
GZ_BLOCK = 65280
SEED = 20250710  # (+ m4; tests/test_edit_overlaps_resident_window_cases.py: every line of these texts is taken)


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e
        e.debug_edit_window(0)


def _fmt(m4):
    return 2 if m4 else 1


def _ingest(engine, text, m4, how="text"):
    if how == "text":
        engine.ingest_text(text, 4, 0.4, fmt=_fmt(m4))
    else:
        engine.ingest_bgzf(ic.bgzf_of(text, level=1), 4, 0.4, fmt=_fmt(m4))


def _resident(engine, op, text, m4, w=W, gz=False):
    """the resident edit in windows of `w` against the restatement: bytes, stats, the windows, the farthest reach, no text ring"""
    engine.debug_edit_window(w)
    got = engine.edit_overlaps_resident(op, NAMES, TYPES, gzip_out=gz)
    want, n_lines, n_kept = restate(text, op, TABLE, m4)
    if gz:
        assert got == engine.gzip(want) and gzip.decompress(got) == want and engine.gzip_stats["in_bytes"] == len(want), (op, m4, len(text))
    else:
        assert got == want, (op, m4, len(text))
    st, ew = engine.edit_stats, engine.edit_windows()
    assert (st["n_lines"], st["n_kept"], st["text_bytes"], st["kept_bytes"]) == (n_lines, n_kept, len(text), len(want))
    assert st["mirror_reused"] == 1 and st["text_ms"] == 0
    assert ew["windows"] == n_windows(text, w) > 1 and ew["max_reach"] == max(window_reaches(text, w)) and ew["text_ring_bytes"] == 0
    return want


# ---- 1. a text of 40 windows, after ingest_text and after ingest_bgzf ---------------------------------------------------------
@pytest.mark.parametrize("how", ["text", "bgzf"])
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_resident_text_of_40_windows(engine, tmp_path, m4, how):
    text = rc.generated(SEED + m4, m4, W)
    assert n_windows(text, W) == 40
    _ingest(engine, text, m4, how)
    for op in OPS:
        for gz in (False, True):
            want = _resident(engine, op, text, m4, gz=gz)
        if op == OP_FILTER:
            assert want == host_loop(str(tmp_path), op, text, NAMES, TYPES, ".m4" if m4 else ".paf")
        # into a file
        engine.debug_edit_window(W)
        out = tmp_path / "res.gz"
        engine.edit_overlaps_resident(op, NAMES, TYPES, out_path=str(out))
        assert out.read_bytes() == engine.gzip(want) and engine.edit_windows()["windows"] == 40
        # the same bytes from the whole-text run, which reports no windows
        engine.debug_edit_window(_NEVER)
        assert engine.edit_overlaps_resident(op, NAMES, TYPES, gzip_out=False) == want and engine.edit_windows()["windows"] == 0
    # W = 3 tiles: a last window of one tile and a bit; W = 5 tiles: C = W = 160 KiB
    for w in (3 * W, 5 * W):
        _resident(engine, OP_FILTER, text, m4, w=w)
        _resident(engine, OP_EXTRACT, text, m4, w=w, gz=True)


# ---- 2. the mirror route: Engine.edit_overlaps on the ingested file itself ----------------------------------------------------
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_edit_from_the_mirror(engine, tmp_path, m4):
    text = rc.generated(SEED + m4, m4, W)
    src, d = tmp_path / ("in" + (".m4" if m4 else ".paf")), tmp_path / "out"
    d.mkdir()
    src.write_bytes(text)
    engine.ingest_paf(str(src), 4, 0.4, fmt=_fmt(m4))
    for op in OPS:
        engine.debug_edit_window(W)
        st = engine.edit_overlaps(op, str(src), str(d / "o.txt"), NAMES, TYPES)
        want, n_lines, n_kept = restate(text, op, TABLE, m4)
        assert (d / "o.txt").read_bytes() == want
        assert (st["mirror_reused"], st["n_lines"], st["n_kept"], st["kept_bytes"]) == (1, n_lines, n_kept, len(want))
        ew = engine.edit_windows()
        assert ew["windows"] == 40 and ew["text_ring_bytes"] == 0 and ew["max_reach"] == max(window_reaches(text, W))
        assert engine.edit_overlaps_resident(op, NAMES, TYPES, gzip_out=False) == want and engine.edit_windows()["windows"] == 40
        os.remove(d / "o.txt")
    # a line that reaches one byte past the look-ahead, begun in window 8: the host loop's, no file
    late = rc.reaching(m4, W, C + 1, bad, lead_windows=9)
    assert rc.windows_take(late, W) is False and window_reaches(late, W)[8] == C + 1
    src.write_bytes(late)
    engine.ingest_paf(str(src), 4, 0.4, fmt=_fmt(m4))
    engine.debug_edit_window(W)
    for op in OPS:
        with pytest.raises(yacrd_amd.NeedsHostParser):
            engine.edit_overlaps(op, str(src), str(d / "o.txt"), NAMES, TYPES)
        assert engine.edit_windows()["windows"] == 0 and os.listdir(d) == []
    # ... and the engine is usable: the same text from the mirror, whole
    engine.debug_edit_window(_NEVER)
    st = engine.edit_overlaps(OP_EXTRACT, str(src), str(d / "o.txt"), NAMES, TYPES)
    assert st["mirror_reused"] == 1 and (d / "o.txt").read_bytes() == restate(late, OP_EXTRACT, TABLE, m4)[0]


# ---- 3. borders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_kept", [True, False], ids=["kept", "dropped"])
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_border_sweep(engine, m4, want_kept):
    """every byte of a line, in turn, is the first byte of window 1; its neighbours have the opposite verdict"""
    for op in OPS:
        cases = rc.border_sweep(m4, W, want_kept, op)
        assert len(cases) == 101
        for cut, text in cases:
            _ingest(engine, text, m4)
            got = _resident(engine, op, text, m4)
            assert (text[W - cut:W - cut + 101] in got) == want_kept, cut
            assert engine.edit_windows()["windows"] == 2 and engine.edit_windows()["max_reach"] == (101 - cut if cut else 0)


@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_look_ahead_edges_and_a_window_without_a_line_start(engine, tmp_path, m4):
    for target in (good, bad):
        text = rc.no_start_window(m4, W, target)
        _ingest(engine, text, m4)
        for op in OPS:
            got = _resident(engine, op, text, m4)
            assert (text[2 * W - 1:3 * W] in got) == ((target is good) == (op == OP_FILTER))
            assert engine.edit_windows()["windows"] == 4 and engine.edit_windows()["max_reach"] == W
    for maker in (good, bad):
        for reach in (C - 1, C):
            for newline in (True, False):  # (without: the last line lacks its newline and lies wholly inside the look-ahead)
                text = rc.reaching(m4, W, reach, maker, newline=newline, behind=newline)
                assert rc.windows_take(text, W)
                _ingest(engine, text, m4, "text" if newline else "bgzf")
                for op in OPS:
                    _resident(engine, op, text, m4)
                    assert engine.edit_windows()["max_reach"] == reach
                _resident(engine, OP_EXTRACT, text, m4, gz=True)
    # one byte more: the text is the host loop's, nothing is written and nothing is left beside the output
    d = tmp_path / "out"
    d.mkdir()
    for newline in (True, False):
        text = rc.reaching(m4, W, C + 1, bad, newline=newline, behind=newline)
        assert rc.windows_take(text, W) is False
        _ingest(engine, text, m4)
        engine.debug_edit_window(W)
        for op in OPS:
            for gz in (False, True):
                with pytest.raises(yacrd_amd.NeedsHostParser):
                    engine.edit_overlaps_resident(op, NAMES, TYPES, gzip_out=gz)
                assert engine.edit_windows()["windows"] == 0
            with pytest.raises(yacrd_amd.NeedsHostParser):
                engine.edit_overlaps_resident(op, NAMES, TYPES, out_path=str(d / "o.gz"))
            assert engine.edit_windows()["windows"] == 0 and os.listdir(d) == []
        # the engine is usable and the text still resident: whole, it is taken
        engine.debug_edit_window(_NEVER)
        assert engine.edit_overlaps_resident(OP_EXTRACT, NAMES, TYPES, gzip_out=False) == restate(text, OP_EXTRACT, TABLE, m4)[0]


@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_last_lines_empty_lines_and_whole_windows(engine, m4):
    for maker in (good, bad):
        other = bad if maker is good else good
        # a last line without its newline, in the last window
        texts = [fill(m4, 2 * W + 100, other) + maker(m4, 200)]
        # empty lines across a border: the border between two newlines, in front of the first, behind the last
        for lead in (W - 2, W - 1, W):
            texts.append(fill(m4, lead, maker) + b"\n\n\n" + fill(m4, W, other))
        # a text of exactly k W and k W +- 1 bytes, with and without its last newline (k W without: the newline it gets
        # opens a tile of its own, behind the mirror's last byte)
        for size in (2 * W - 1, 2 * W, 2 * W + 1, 3 * W):
            whole = fill(m4, size - 300, other) + maker(m4, 299) + b"\n"
            texts += [whole, whole[:-1]]
        for i, text in enumerate(texts):
            _ingest(engine, text, m4, "bgzf" if i & 1 else "text")
            for op in OPS:
                _resident(engine, op, text, m4)
            _resident(engine, OP_FILTER if maker is good else OP_EXTRACT, text, m4, gz=True)


# ---- 4. gzip out --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m4", [False, True], ids=["paf", "m4"])
def test_gzip_out_windows_that_keep_nothing(engine, m4):
    # a tail of 1000 bytes is handed through five windows that keep nothing, then encoded with what the last ones keep
    text = fill(m4, 1000, good) + fill(m4, 6 * W, bad) + fill(m4, W + 4000, good)
    _ingest(engine, text, m4)
    assert len(_resident(engine, OP_FILTER, text, m4, gz=True)) == W + 5000
    assert len(_resident(engine, OP_EXTRACT, text, m4, gz=True)) == 6 * W
    # kept bytes that end exactly on a block's border, one byte before and one behind it
    for d in (-1, 0, 1):
        text = fill(m4, 2 * GZ_BLOCK + d, good) + fill(m4, 2 * W, bad)
        _ingest(engine, text, m4)
        assert len(_resident(engine, OP_FILTER, text, m4, gz=True)) == 2 * GZ_BLOCK + d
    # nothing kept at all: the EOF member alone
    nothing = fill(m4, 5 * W + 17, bad)
    _ingest(engine, nothing, m4)
    assert _resident(engine, OP_FILTER, nothing, m4, gz=True) == b"" and len(engine.gzip(b"")) == 28


# ---- 5. bounded footprint -----------------------------------------------------------------------------------------------------
def test_only_the_output_ring_is_held():
    before = live_bytes()
    with yacrd_amd.Engine(device_id=0) as e:
        rings = []
        for windows in (20, 40):
            text = fill(False, windows * W - 123, good)[:-1]
            e.debug_edit_window(W)
            assert e.edit_overlaps_text(OP_FILTER, text, NAMES, TYPES, 1) == text + b"\n"  # (a plain run first: it leaves text slots)
            assert e.edit_windows()["text_ring_bytes"] > 2 * W
            e.ingest_text(text, 4, 0.4)
            assert e.edit_overlaps_resident(OP_FILTER, NAMES, TYPES, gzip_out=False) == text + b"\n"
            assert gzip.decompress(e.edit_overlaps_resident(OP_FILTER, NAMES, TYPES)) == text + b"\n"
            ew = e.edit_windows()
            assert ew["windows"] == windows and ew["text_ring_bytes"] == 0  # (the plain run's text slots have gone)
            rings.append(ew["out_ring_bytes"])
        assert rings[0] == rings[1] and 2 * W < rings[0] <= 2 * (W + GZ_BLOCK + 64) * 1.125
        text = fill(False, 80 * W, bad)
        e.ingest_text(text, 4, 0.4)
        e.trim()
        # (what the engine keeps whatever is trimmed: the mover's pinned arena, the bounce buffers, the batch path's buffers
        # the ingest of this very text ran its sweep in)
        warm = live_bytes()
        e.ingest_text(text, 4, 0.4)
        held_ingest = live_bytes()
        assert e.edit_overlaps_resident(OP_EXTRACT, NAMES, TYPES, gzip_out=False) == text and e.edit_windows()["windows"] == 80
        held = live_bytes()
        # (beside the ingest's buffers: the plain output ring — two slots of W + 64 — and the tables, less than the text)
        assert held_ingest[0] + 2 * W < held[0] < held_ingest[0] + len(text)
        e.trim()
        assert live_bytes() == warm
    assert live_bytes() == before


# ---- 6. the CLI ---------------------------------------------------------------------------------------------------------------
def _cli(args, **env):
    base = {k: v for k, v in os.environ.items() if k not in ("YACRD_DEVICE_INFLATE", "YACRD_NO_DEVICE_INFLATE", "YACRD_EDIT_WINDOW")}
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(base, **env))
    assert p.returncode == 0, p.stderr
    return p


def _editor_line(stream):
    hit = [l for l in stream.splitlines() if l.startswith("[info] device editor")]
    assert len(hit) == 1, stream
    return hit[0]


@pytest.mark.parametrize("op", ["filter", "extract"])
@pytest.mark.parametrize("form", ["plain", "bgzf"])
def test_cli_on_the_detections_own_file(golden_dir, tmp_path, op, form):
    """W = 32 768: no multiple of it is a window border of another kind (the mover's chunk, the encoder's block)"""
    text = open(os.path.join(golden_dir, "reads.paf"), "rb").read()
    ext = ".paf" if form == "plain" else ".paf.gz"
    x = tmp_path / ("x" + ext)
    if form == "plain":
        shutil.copy(os.path.join(golden_dir, "reads.paf"), x)
    else:
        x.write_bytes(ic.bgzf_of(text, level=6))
    more = {} if form == "plain" else {"YACRD_DEVICE_INFLATE": "1"}  # (the detection ingests the BGZF file on the device: the text is resident)

    def run(tag, **env):
        out = tmp_path / (tag + ext)
        p = _cli(["-i", x, "-o", tmp_path / (tag + ".yacrd"), "-c", "4", "-n", "0.4", op, "-i", x, "-o", out], YACRD_CLI_TIMING="1", **env)
        return p, out.read_bytes()

    p, got = run("win", YACRD_EDIT_WINDOW=str(W), **more)
    q, whole = run("whole", YACRD_EDIT_WINDOW=str(_NEVER), **more)
    h, host_out = run("host", YACRD_NO_DEVICE_EDITOR="1")
    assert "[info] device editor" not in h.stderr + h.stdout
    lp, lq = (_editor_line(r.stderr if form == "plain" else r.stdout) for r in (p, q))
    assert ("mirror_reused=1" if form == "plain" else "resident=1 device_inflate=1") in lp, lp
    assert int(lp.rsplit(" windows=", 1)[1]) == n_windows(text, W) > 1 and lq.endswith(" windows=0"), (lp, lq)
    assert got == whole and len(got) > 0
    inflate = (lambda b: b) if form == "plain" else gzip.decompress
    assert inflate(got) == inflate(host_out)
    assert 0 < len(inflate(got)) < len(text) and inflate(got).count(b"\n") == (1286 - 448 if op == "filter" else 448)
