"""What tests/test_edit_fasta_window_cases.py (CPU) and tests/test_gpu_edit_fasta_windows.py (GPU) share: the FASTA editor's
windows (csrc/gpu_seq_edit.hip: run_windows) restated — which texts a run in windows of W bytes takes, what every
window carries into the next —, a seeded generator of texts that span tens of windows over one table of about 2 000 reads,
and the fixed texts of the windows' own edges.  The bytes' yardsticks are edit_fasta_cases.restate and the host loop."""
import random

from edit_fasta_cases import _WIDTHS, lay_out
from edit_fastq_cases import Table, _bases, _regions, _SHAPES, _token

TILE = 32768
W_SMALL = 32768   # the window of the generated texts' GPU tests: one tile, the smallest there is
MAX_BASES = 10000  # the table's longest read: at width 1 with blank lines behind every line still a record of less than W_SMALL


def _lines(text):
    """(start, end) of every line that has its newline; end is the byte behind the newline"""
    out, at = [], 0
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            return out
        out.append((at, nl + 1))
        at = nl + 1


def record_spans(text):
    """-> (front, [bytes of every record]): a record is a header line — one whose first byte is '>' — through the last line in
    front of the next header, blank lines and a last line without its newline among them; `front` is what stands in front of
    the first header, that header's line included (the whole text where there is none)"""
    heads = [s for s, e in _lines(text) if text[s:s + 1] == b">"]
    tail = _lines(text)[-1][1] if b"\n" in text else 0
    if tail < len(text) and text[tail:tail + 1] == b">":
        heads.append(tail)
    if not heads:
        return len(text), []
    nl = text.find(b"\n", heads[0])
    return (nl + 1 if nl >= 0 else len(text)), [b - a for a, b in zip(heads, heads[1:] + [len(text)])]


def windows_take(text, W):
    """The rule of the windows, from the records alone.  True: a run in windows of W bytes takes `text` (as far as the windows
    go: what the records hold is edit_fasta_cases.device_takes' matter); False: it hands the text to the host loop; None:
    either is right.  A record of at most W bytes is always taken, one of more than 2 W never; a last line without its
    newline never.  What stands in front of the first header is carried until that header's line is whole: up to 2 W bytes
    with the line, never more."""
    if not text:
        return True
    if not text.endswith(b"\n"):
        return False
    front, recs = record_spans(text)
    if front > 2 * W:
        return False
    longest = max(recs, default=0)
    return True if longest <= W else False if longest > 2 * W else None


def window_carries(text, W):
    """The run itself, window by window: window k's text is the carry of window k - 1 and then text[k W, (k + 1) W).  Of its
    whole lines H begin with '>'; a window that is not the last completes max(H - 1, 0) records and carries everything from
    the first byte of its last header line on — all of it with H = 0 —, a partial last line included.  Nothing in a window
    says that its last record is whole but a partial last line that begins with '>': then (H > 0) all H records are
    complete and that line alone is carried, so that a record of W bytes with a '>' behind it still leaves a carry of at
    most W.  The last window completes H records and must end with a newline.  -> the carries of the windows but the last,
    or None when one is longer than W (the carry area) or the text's last newline is missing."""
    carries, carry = [], b""
    n_win = (len(text) + W - 1) // W
    for k in range(n_win):
        win = carry + text[k * W:(k + 1) * W]
        if k + 1 == n_win:
            return carries if win.endswith(b"\n") else None
        lines = _lines(win)
        heads = [s for s, e in lines if win[s:s + 1] == b">"]
        partial = win[lines[-1][1]:] if lines else win
        carry = win if not heads else partial if partial.startswith(b">") else win[heads[-1]:]
        if len(carry) > W:
            return None
        carries.append(len(carry))
    return carries


def n_windows(text, W):
    """the windows a run with the switch at W reports: none for a text of at most one window"""
    return (len(text) + W - 1) // W if len(text) > W else 0


# ---- fixed builders -----------------------------------------------------------------------------------------------------------
def filler(size):
    """one record `>f` (`>ff` where the arithmetic asks for it), absent from every table, of exactly `size` bytes (>= 3), its
    bases 80 a line: what the editors write back as it stands"""
    return record_of(size, b"f", pad=b"f", base=b"A")


def fillers(total, each=1019):
    """records `>f` of `each` bytes, `total` bytes in all (>= 3): the last takes what is left"""
    n = max(0, total // each - 1)
    return filler(each) * n + filler(total - n * each)


def record_of(size, name=b"big", width=80, desc=b"", pad=b"x", base=b"G"):
    """one record of exactly `size` bytes: `>name[ desc]` and bases on lines of `width`, the last line shorter (the name a
    byte longer, by `pad`, where a last line would be a newline alone); the name is absent from the generator's table"""
    for p in (b"", pad):
        head = b">" + name + p + (b" " + desc if desc else b"") + b"\n"
        m = size - len(head)
        rows, rest = divmod(m, width + 1)
        if rest != 1 and m >= 0:
            rec = head + (base * width + b"\n") * rows + (base * (rest - 1) + b"\n" if rest else b"")
            assert len(rec) == size, (size, len(rec))
            return rec
    raise AssertionError(size)


def long_record_text(W):
    """three good windows, then one record of 2 W + 1 bytes: never taken"""
    return fillers(3 * W - 9) + record_of(2 * W + 1) + filler(101)


def blank_front_text(W, tail=b""):
    """W + 1 blank lines, then the first header: what stands in front of it spans the border of windows 0 and 1"""
    return b"\n" * (W + 1) + b">first one\nACGT\nAC\n" + tail


# ---- the generator ---------------------------------------------------------------------------------------------------------
def window_table(seed=20261020, n_reads=2000):
    """one table for every generated text: reads of 0 to MAX_BASES bases, regions of every shape, types set freely"""
    rng = random.Random(seed)
    names, lens, regs, types = [], [], [], []
    seen = set()
    while len(names) < n_reads:
        name = b"r%d/" % len(names) + _token(rng, rng.choice([0, 1, 3, 9, 40]))
        if name in seen:
            continue
        seen.add(name)
        length = rng.choice([0, 1, 2, 10, 79, 80, 81, 159, 160, 161, 500, 1000, 2999, MAX_BASES, rng.randint(0, 3000)])
        names.append(name), lens.append(length), regs.append(_regions(rng, rng.choice(_SHAPES), length)), types.append(rng.randint(0, 2))
    return Table(names, lens, regs, types)


def window_text(table, seed, n_bytes):
    """records over `table` until the text holds n_bytes: names of the table and absent ones, descriptions behind a blank, a
    tab or a form feed, every layout of edit_fasta_cases._WIDTHS, blank lines inside and behind records, zero-length records"""
    rng = random.Random(seed)
    out, size = [b"\n\n"], 2  # (blank lines in front of the first header)
    while size < n_bytes:
        x = rng.random()
        if x < 0.06:
            rec = b">f\n"  # a record of no line at all
        else:
            if x < 0.25:
                name, n = b"absent%d" % rng.randint(0, 99), rng.randint(0, 3000)
            else:
                i = rng.randrange(len(table.names))
                name, n = table.names[i], table.lengths[i]
            head = b">" + name
            u = rng.random()
            if u < 0.1:
                head += rng.choice([b" ", b"\t", b"\x0c"])  # an empty description behind its separator
            elif u < 0.55:
                head += rng.choice([b" ", b"\t", b"\x0c"]) + _token(rng, rng.randint(1, 30)) + (b" x\ty" if rng.random() < 0.3 else b"")
            rec = head + b"\n" + lay_out(rng, _bases(rng, n), rng.choice(_WIDTHS), blanks=0.15 if rng.random() < 0.3 else 0.0)
            if rng.random() < 0.15:
                rec += b"\n" * rng.randint(1, 2)  # blank lines behind a record
        out.append(rec)
        size += len(rec)
    return b"".join(out)


def window_cases(n_bytes=40 * W_SMALL):
    """(tag, text, Table): texts of about 40 windows of W_SMALL, every one taken for all four ops"""
    table = window_table()
    for k in range(2):
        yield "gen%d" % k, window_text(table, 2000 + k, n_bytes), table
