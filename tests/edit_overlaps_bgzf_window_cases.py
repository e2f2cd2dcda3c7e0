"""What tests/test_edit_overlaps_bgzf_window_cases.py (CPU) and tests/test_gpu_edit_overlaps_bgzf_windows.py (GPU) share: the
overlap editor's windows over a BGZF text (csrc/gpu_edit.hip: bgzf_windows_loop) restated from the stream's cuts
(edit_bgzf_window_cases.cuts_of: csrc/bgzf_windows.h restated) and the text alone — the windows are the cuts that hold text,
window j sees ahead_j = min(C, L_{j+1}) bytes of the next one, and a line that starts in window j is taken iff it ends inside
them — and builders of streams that put a window's end where a case wants it.  Lines and tables: edit_overlaps_window_cases."""
import random

import numpy as np

from edit_bgzf_window_cases import W_BGZF, cuts_of, drawn_sizes, stream_of  # noqa: F401 (re-exported)
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, TILE, restate  # noqa: F401 (re-exported)
from edit_overlaps_window_cases import NAMES, TABLE, TYPES, _line_spans, bad, chunk_of, fill, generated, good  # noqa: F401

W_TEST = W_BGZF  # 65 536: the smallest window of a BGZF run, so C = 65 536 as well
SWEEP_NEXT = 50000  # border_sweep: the bytes of window 1


def bgzf_window(switch):
    """the window of a BGZF run for what Engine.debug_edit_window holds (a number of bytes): rounded up to a tile, at least 64 KiB"""
    return max((switch + TILE - 1) // TILE * TILE, W_BGZF)


def windows_of(cuts, W):
    """-> [(t0, t1, ahead)]: the cuts that hold text, each with the bytes of the next one it sees (the last: 0)"""
    C = chunk_of(W)
    spans = [(c[4], c[5]) for c in cuts if c[5] > c[4]]
    return [(t0, t1, min(C, spans[j + 1][1] - spans[j + 1][0]) if j + 1 < len(spans) else 0) for j, (t0, t1) in enumerate(spans)]


def window_reaches(text, wins):
    """per window: how many bytes of the text a line that began in it has behind the window's end, at most (0: none does)"""
    out = [0] * len(wins)
    if not text or not wins:
        return out
    s, e = _line_spans(text)
    ends = np.asarray([w[1] for w in wins], np.int64)
    j = np.searchsorted(ends, s, side="right")  # (the window a line starts in: the first whose end lies behind its first byte)
    reach = np.maximum(e - ends[j], 0)
    for jj, r in zip(j[reach > 0].tolist(), reach[reach > 0].tolist()):
        out[jj] = max(out[jj], r)
    return out


def refused(text, wins):
    """the windows that hold a line the run in windows does not take: one that reaches beyond the window's look-ahead"""
    return [j for j, (r, w) in enumerate(zip(window_reaches(text, wins), wins)) if j + 1 < len(wins) and r > w[2]]


def windows_take(text, blob, W):
    """True / False as edit_overlaps_window_cases.windows_take; None: a '"' or a CR"""
    if b'"' in text or b"\r" in text:
        return None
    return not refused(text, windows_of(cuts_of(blob, W), W))


# ---- streams -------------------------------------------------------------------------------------------------------------------
def own_stream(text, kind="level1", eof=True):
    """members of 65 280 bytes of text: what the project's own encoder writes"""
    sizes = [65280] * (len(text) // 65280) + ([len(text) % 65280] if len(text) % 65280 else [])
    return stream_of(text, sizes, kind, eof)


def drawn(text, seed):
    """members of drawn sizes (none so small in front of one so large that a window of a few bytes arises: the generated
    texts' lines must all be taken) and drawn kinds"""
    rng = random.Random(seed)
    sizes = drawn_sizes(rng, len(text), choices=(4093, 32768, 65279, 65280), p_random=0.3)
    kinds = [rng.choice(("stored", "level1", "level6")) for _ in sizes]
    return stream_of(text, sizes, kinds)


def with_windows(text, lens, kind="stored", eof=True, empties=()):
    """one member per window: `lens` are the windows' bytes (they sum to the text's; any two neighbours sum to more than
    65 536, so no window can take the next one's member).  `empties`: windows in front of which an EOF member is put
    (it joins the window before it, or the one behind it: an empty member mid-stream).  -> the stream"""
    assert sum(lens) == len(text) and all(0 < n <= W_BGZF for n in lens), lens
    assert all(a + b > W_BGZF for a, b in zip(lens, lens[1:])), lens
    sizes = []
    for j, n in enumerate(lens):
        sizes += ([0] if j in empties else []) + [n]
    blob = stream_of(text, sizes, kind, eof)
    got = [c[5] - c[4] for c in cuts_of(blob, W_BGZF) if c[5] > c[4]]
    assert got == list(lens), (lens, got)
    return blob


def border_sweep(m4, off, want_kept, op):
    """Window 0 ends at tile offset `off` of its second tile (T = 32 768 + off; off 0: at 65 536, the tile's own end).  A target
    line of 100 bytes and its newline whose every byte is in turn the first byte of window 1, between lines of the opposite
    verdict.  -> [(cut, text, T)]"""
    T = TILE + off if off else 2 * TILE
    keeps = lambda maker: (maker is good) == (op == OP_FILTER)
    target = (good if keeps(good) == want_kept else bad)(m4, 100) + b"\n"
    other = bad if keeps(good) == want_kept else good
    before, after = other(m4) + b"\n", other(m4) + b"\n"
    out = []
    for cut in range(len(target)):
        head = fill(m4, T - cut - len(before), good if cut & 1 else bad) + before
        text = head + target + after
        text += fill(m4, T + SWEEP_NEXT - len(text), bad if cut & 2 else good)
        assert len(head) + cut == T
        out.append((cut, text, T))
    return out


def reaching(m4, T, reach, maker=bad, start_back=50, newline=True, behind=1000):
    """a line that begins `start_back` bytes in front of text position T and has `reach` bytes (its newline counted, where it
    has one) behind T; lines of the other verdict in front of it and, `behind` bytes of them, behind it"""
    other = bad if maker is good else good
    body = maker(m4, start_back + reach - (1 if newline else 0)) + (b"\n" if newline else b"")
    text = fill(m4, T - start_back, other) + body
    if behind:
        assert newline
        text += fill(m4, behind, other)
    return text
