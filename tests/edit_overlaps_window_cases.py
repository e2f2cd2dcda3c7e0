"""What tests/test_edit_overlaps_window_cases.py (CPU) and tests/test_gpu_edit_overlaps_windows.py (GPU) share: the overlap
editor's windows (csrc/gpu_edit.hip: windows_loop) restated from the bytes alone — which texts a run in windows of W
bytes takes, how far a line reaches into the next window — and the texts that put lines on the windows' borders.  Lines,
ids and tables come from edit_overlaps_cases."""
import random

import numpy as np

from edit_overlaps_cases import CHUNK, OP_EXTRACT, OP_FILTER, TILE, _line, _pool, _sized, restate  # noqa: F401 (re-exported)

W_TEST = TILE  # the tests' window: one tile, so the look-ahead C is one tile as well


def chunk_of(W):
    """the mover's chunk in a run in windows of W bytes: how far window k's marks see into window k + 1"""
    return min(CHUNK, W)


def n_windows(text, W):
    return (len(text) + W - 1) // W


def _line_spans(text):
    """-> (first byte, one past the last real byte) of every line, its newline included where it has one"""
    n = len(text)
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10).astype(np.int64)
    starts = np.concatenate(([0], nl + 1))
    ends = np.concatenate((nl + 1, [n]))
    live = starts < n  # (behind a final newline no line begins)
    return starts[live], ends[live]


def window_reaches(text, W):
    """per window: how many bytes of the text a line that began in it has in the windows behind it, at most (0: none does)"""
    out = [0] * n_windows(text, W)
    if not text:
        return out
    s, e = _line_spans(text)
    k = s // W
    reach = np.maximum(e - (k + 1) * W, 0)
    for kk, r in zip(k[reach > 0].tolist(), reach[reach > 0].tolist()):
        out[kk] = max(out[kk], r)
    return out


def windows_take(text, W):
    """True: every line ends within C bytes past the end of the window it starts in — the run in windows takes the text.
    False: some line reaches farther — YACRD_EFALLBACK, nothing written.  None: the text is not the windows' to decide
    (a '"' or a CR: the editor hands it back whatever the route; field counts are the caller's to keep equal)."""
    if b'"' in text or b"\r" in text:
        return None
    return max(window_reaches(text, W), default=0) <= chunk_of(W)


# ---- tables and lines with a known verdict ----------------------------------------------------------------------------------
NAMES = [b"good_a", b"good_b", b"bad_nc", b"bad_ch"]
TYPES = [0, 0, 1, 2]
TABLE = dict(zip(NAMES, TYPES))


def line_of(m4, a, b, size=None):
    """one line without its newline, ids `a` and `b`; stretched by its last column to `size` bytes where given"""
    if m4:
        l = b"%s %s 0.1 2 0 100 450 1000 0 550 900 1000" % (a, b)
    else:
        l = b"%s\t12000\t20\t4500\t-\t%s\t10000\t5500\t10000\t4500\t4500\t255" % (a, b)
    if size is not None:
        assert size >= len(l), (size, len(l))
        l += b"7" * (size - len(l))
    return l


def good(m4, size=None):
    """both reads good: filter keeps it, extract drops it"""
    return line_of(m4, b"good_a", b"absent", size)


def bad(m4, size=None):
    """two ids of the table with different types, one of them bad: filter drops it, extract keeps it"""
    return line_of(m4, b"good_b", b"bad_ch", size)


def fill(m4, size, maker=good):
    """exactly `size` bytes of whole lines of `maker`'s verdict (size 0: nothing; else at least one short line)"""
    if size == 0:
        return b""
    unit = maker(m4) + b"\n"
    assert size >= len(unit), size
    k = size // len(unit) - 1
    return unit * k + maker(m4, size - k * len(unit) - 1) + b"\n"


def generated(seed, m4, W, windows=40):
    """-> (text, names, types): a fuzz text of edit_overlaps_cases' lines that ends 777 bytes short of `windows` windows"""
    rng = random.Random(seed)
    ids, known, types = _pool(rng)
    return _sized(rng, ids, rng.randint(9, 17), m4, windows * W - 777), known, types


def border_sweep(m4, W, want_kept, op):
    """Two windows; a target line of about 100 bytes whose every byte is in turn the first of window 1 (the cut falls inside
    its first id, on the delimiters, inside id b, on the newline), between two lines of the opposite verdict.
    -> [(cut, text)], cut = the target's byte that window 1 begins with."""
    keeps = lambda maker: (maker is good) == (op == OP_FILTER)
    target = (good if keeps(good) == want_kept else bad)(m4, 100) + b"\n"
    other = bad if keeps(good) == want_kept else good
    before, after = other(m4) + b"\n", other(m4) + b"\n"
    out = []
    for cut in range(len(target)):
        head = fill(m4, W - cut - len(before), good if cut & 1 else bad) + before
        text = head + target + after
        text += fill(m4, 2 * W - 300 - len(text), bad if cut & 2 else good)
        assert len(head) + cut == W and W < len(text) <= 2 * W
        out.append((cut, text))
    return out


def no_start_window(m4, W, target):
    """a line that begins at the last byte of window 1 and whose newline is the last byte of window 2 — window 2 has no line
    start —, of `target`'s verdict, between lines of the opposite one; four windows"""
    other = bad if target is good else good
    text = fill(m4, 2 * W - 1, other) + target(m4, W) + b"\n" + fill(m4, W - 5, other)
    assert text[2 * W - 2:2 * W - 1] == b"\n" and text[3 * W - 1:3 * W] == b"\n" and b"\n" not in text[2 * W - 1:3 * W - 1]
    return text


def reaching(m4, W, reach, maker=bad, start_back=50, newline=True, behind=True):
    """a line that begins `start_back` bytes in front of the end of window 0 and has `reach` bytes (its newline counted, where
    it has one) in the windows behind it; lines of the other verdict around it (none behind it where `behind` is false)"""
    other = bad if maker is good else good
    body = maker(m4, start_back + reach - (1 if newline else 0)) + (b"\n" if newline else b"")
    text = fill(m4, W - start_back, other) + body
    if behind:
        assert newline
        text += fill(m4, 1000, other)
    assert window_reaches(text, W)[0] == reach
    return text
