"""What tests/test_edit_fastq_window_cases.py (CPU) and tests/test_gpu_edit_fastq_windows.py (GPU) share: the FASTQ editor's
windows (csrc/gpu_seq_edit.hip: run_windows) restated — which texts a run in windows of W bytes takes, what every
window carries into the next —, a seeded generator of texts that span tens of windows over one table of about 2 000 reads,
and the texts that must fall back late.  The bytes' yardsticks are edit_fastq_cases.restate and the host loop."""
import random

from edit_fastq_cases import Table, _bases, _regions, _SHAPES, _token

TILE = 32768
W_SMALL = 32768  # the window of the generated texts' GPU tests: one tile, the smallest there is


def _record_lengths(text):
    """the bytes of every record (four lines each) of a text whose line count is a multiple of four"""
    ends, at = [], -1
    while True:
        at = text.find(b"\n", at + 1)
        if at < 0:
            break
        ends.append(at)
    return [ends[i + 3] - (ends[i - 1] if i else -1) for i in range(0, len(ends) - 3, 4)]


def windows_take(text, W):
    """The rule of the windows, from the records alone.  True: a run in windows of W bytes takes `text` (as far as the windows
    go: what the records hold is edit_fastq_cases.device_takes' matter); False: it hands the text to the host loop; None:
    either is right.  A record of at most W bytes is always taken, one of more than 2 W never; a last line without its
    newline, or a line count that is no multiple of four, never."""
    if not text:
        return True
    if not text.endswith(b"\n") or text.count(b"\n") % 4:
        return False
    longest = max(_record_lengths(text))
    return True if longest <= W else False if longest > 2 * W else None


def window_carries(text, W):
    """The run itself, window by window: window k's text is the carry of window k - 1 and then text[k W, (k + 1) W); it
    completes floor(lines / 4) records, what lies behind them is its carry.  -> the carries of the windows but the last, or
    None when one is longer than W (the carry area) or the last window does not end on a record."""
    carries, carry = [], b""
    n_win = (len(text) + W - 1) // W
    for k in range(n_win):
        win = carry + text[k * W:(k + 1) * W]
        at, lines, done = -1, 0, 0
        while True:
            at = win.find(b"\n", at + 1)
            if at < 0:
                break
            lines += 1
            if lines % 4 == 0:
                done = at + 1
        carry = win[done:]
        if k + 1 < n_win:
            if len(carry) > W:
                return None
            carries.append(len(carry))
        elif carry:
            return None
    return carries


def filler(size):
    """records `@f`, absent from every table, of exactly `size` bytes (7, or >= 14): one record is 2 m + 7 bytes"""
    if size % 2 == 0:
        return b"@f\n\n+\n\n" + filler(size - 7)
    m = (size - 7) // 2
    assert m >= 0
    return b"@f\n" + b"A" * m + b"\n+\n" + b"#" * m + b"\n"


def fillers(total, each=1019):
    """records `@f` of `each` bytes (odd), `total` bytes in all: the last one or two take what is left"""
    n = max(0, total // each - 1)
    return filler(each) * n + filler(total - n * each)


def record_of(size, name=b"big"):
    """one record of exactly `size` bytes, its name (a byte longer where the parity asks for it) absent from the generator's table"""
    if (size - len(name)) % 2:
        name += b"x"
    m = (size - len(name) - 6) // 2
    rec = b"@" + name + b"\n" + b"C" * m + b"\n+\n" + b"$" * m + b"\n"
    assert len(rec) == size, (size, len(rec))
    return rec


# ---- the generator ---------------------------------------------------------------------------------------------------------
def window_table(seed=20261020, n_reads=2000):
    """one table for every generated text: reads of 0 to 3 000 bases, regions of every shape, types set freely"""
    rng = random.Random(seed)
    names, lens, regs, types = [], [], [], []
    seen = set()
    while len(names) < n_reads:
        name = b"r%d/" % len(names) + _token(rng, rng.choice([0, 1, 3, 9, 40]))
        if name in seen:
            continue
        seen.add(name)
        length = rng.choice([0, 1, 2, 10, 79, 80, 81, 500, 1000, 2999, 3000, rng.randint(0, 3000)])
        names.append(name), lens.append(length), regs.append(_regions(rng, rng.choice(_SHAPES), length)), types.append(rng.randint(0, 2))
    return Table(names, lens, regs, types)


def _quality(rng, n):
    q = bytearray(_bases(rng, n).translate(bytes.maketrans(b"ACGT", b"5I#~")))
    if n and rng.random() < 0.4:
        q[0] = rng.choice(b"@+")  # a quality line that looks like a header or a separator
    return bytes(q)


def window_text(table, seed, n_bytes):
    """records over `table` until the text holds n_bytes: names of the table and absent ones, descriptions, quality lines that
    begin with '@' and with '+', empty records"""
    rng = random.Random(seed)
    out, size = [], 0
    while size < n_bytes:
        x = rng.random()
        if x < 0.06:
            rec = b"@f\n\n+\n\n"
        else:
            if x < 0.25:
                name, n = b"absent%d" % rng.randint(0, 99), rng.randint(0, 3000)
            else:
                i = rng.randrange(len(table.names))
                name, n = table.names[i], table.lengths[i]
            desc = b" " + _token(rng, rng.randint(1, 30)) + (b" x y" if rng.random() < 0.3 else b"") if rng.random() < 0.5 else b""
            rec = b"@" + name + desc + b"\n" + _bases(rng, n) + b"\n+\n" + _quality(rng, n) + b"\n"
        out.append(rec)
        size += len(rec)
    return b"".join(out)


def window_cases(n_bytes=40 * W_SMALL):
    """(tag, text, Table): texts of about 40 windows of W_SMALL, every one taken for all four ops"""
    table = window_table()
    for k in range(2):
        yield "gen%d" % k, window_text(table, 1000 + k, n_bytes), table


# ---- what must fall back: the windows' own causes ------------------------------------------------------------------------------
def long_record_text(W):
    """three good windows, then one record of 2 W + 1 bytes: never taken"""
    return fillers(3 * W - 9) + record_of(2 * W + 1) + filler(101)


def missing_line_texts(text, W):
    """(tag, text'): `text` (more than three windows) with one line deleted in window 2, and without its last newline"""
    at = text.index(b"\n", 2 * W + W // 2)
    return [("line_deleted", text[:at] + text[text.index(b"\n", at + 1):]), ("no_final_newline", text[:-1])]
