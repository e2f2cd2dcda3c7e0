"""What tests/test_edit_overlaps_resident_window_cases.py (CPU) and tests/test_gpu_edit_overlaps_resident_windows.py (GPU)
share: texts for the overlap editor's windows over a text that is RESIDENT (csrc/gpu_edit.hip: windows_loop from the mirror;
DESIGN 7o).  The windows' rule is 7n's — window k is bytes [k W, (k + 1) W), a line may end up to C bytes into the next one —
and is restated in edit_overlaps_window_cases; what differs is that the text has to pass an INGEST first, so every line here
is a record the device parser takes: decimal columns, and a line is stretched by leading zeros in its last column (a mapq of
000...255, a length of 000...1000), never by another digit."""
import random

from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, TILE, restate  # noqa: F401 (re-exported)
from edit_overlaps_window_cases import chunk_of, n_windows, window_reaches, windows_take  # noqa: F401 (re-exported)

W_TEST = TILE  # the tests' window: one tile, so the look-ahead C is one tile as well (the CLI test's 32 768 too)

# the edit's type table: independent of what the ingest makes of the text.  `absent` is in no table: NotBad.
NAMES = [b"good_a", b"good_b", b"bad_nc", b"bad_ch", b"g"]
TYPES = [0, 0, 1, 2, 0]
TABLE = dict(zip(NAMES, TYPES))
_LEN = {b"good_a": 12000, b"good_b": 12001, b"bad_nc": 12002, b"bad_ch": 12003, b"g": 12004, b"absent": 12005}


def line_of(m4, a, b, size=None):
    """one record without its newline, ids `a` and `b`, every read with one length wherever it stands; stretched by
    leading zeros in its last column to `size` bytes where given"""
    la, lb = _LEN[a], _LEN[b]
    if m4:
        head, last = b"%s %s 0.1 2 0 100 450 %d 0 550 900 " % (a, b, la), b"%d" % lb
    else:
        head, last = b"%s\t%d\t20\t4500\t-\t%s\t%d\t5500\t10000\t4500\t4500\t" % (a, la, b, lb), b"255"
    if size is not None:
        assert size >= len(head) + len(last), (size, len(head) + len(last))
        last = b"0" * (size - len(head) - len(last)) + last
    return head + last


def good(m4, size=None):
    """both reads good: filter keeps it, extract drops it"""
    return line_of(m4, b"good_a", b"absent", size)


def bad(m4, size=None):
    """two ids of the table, one of them bad: filter drops it, extract keeps it"""
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
    """-> a text of records over all the ids, in both places, kept and dropped in no order, with empty lines among them, that
    ends 777 bytes short of `windows` windows (its last line stretched to fit)"""
    rng = random.Random(seed)
    ids = sorted(_LEN)
    size = windows * W - 777
    parts, have = [], 0
    while True:
        a, b = rng.choice(ids), rng.choice(ids)
        l = line_of(m4, a, b) + b"\n"
        if rng.random() < 0.2:  # (lines of many lengths: the borders fall everywhere in them)
            l = line_of(m4, a, b, len(l) - 1 + rng.randint(0, 300)) + b"\n"
        if have + len(l) + 400 > size:
            break
        parts.append(l)
        have += len(l)
        if rng.random() < 0.03:
            parts.append(b"\n")
            have += 1
    parts.append(line_of(m4, rng.choice(ids), rng.choice(ids), size - have - 1) + b"\n")
    text = b"".join(parts)
    assert len(text) == size
    return text


def border_sweep(m4, W, want_kept, op):
    """edit_overlaps_window_cases.border_sweep with this module's lines: two windows; every byte of a target line of 100
    bytes and its newline is in turn the first byte of window 1, between two lines of the opposite verdict.
    -> [(cut, text)]"""
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


def reaching(m4, W, reach, maker=bad, start_back=50, newline=True, behind=True, lead_windows=1):
    """a line that begins `start_back` bytes in front of the end of window `lead_windows - 1` and has `reach` bytes (its
    newline counted, where it has one) in the windows behind it; lines of the other verdict around it (none behind it where
    `behind` is false)"""
    other = bad if maker is good else good
    body = maker(m4, start_back + reach - (1 if newline else 0)) + (b"\n" if newline else b"")
    text = fill(m4, lead_windows * W - start_back, other) + body
    if behind:
        assert newline
        text += fill(m4, 1000, other)
    assert window_reaches(text, W)[lead_windows - 1] == reach
    return text


def no_start_window(m4, W, target):
    """a line that begins at the last byte of window 1 and whose newline is the last byte of window 2 — window 2 has no line
    start —, of `target`'s verdict, between lines of the opposite one; four windows"""
    other = bad if target is good else good
    text = fill(m4, 2 * W - 1, other) + target(m4, W) + b"\n" + fill(m4, W - 5, other)
    assert text[2 * W - 2:2 * W - 1] == b"\n" and text[3 * W - 1:3 * W] == b"\n" and b"\n" not in text[2 * W - 1:3 * W - 1]
    return text
