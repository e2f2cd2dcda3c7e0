"""What tests/test_edit_fasta_cases.py (CPU) and tests/test_gpu_edit_fasta.py (GPU) share: the four editors' rules restated
over FASTA records (include/yacrd_engine.h: yacrd_engine_edit_fasta), which texts the device editor takes, the seeded case
generator and the set of texts that must fall back.  The host loop (host.edit_file on a ".fasta") is the yardstick for bytes;
the table, the cut positions and the region shapes are those of edit_fastq_cases."""
import random
import re

from edit_fastq_cases import (CHIMERIC, NOT_BAD, NOT_COVERED, OPS, OP_EXTRACT, OP_FILTER, OP_SCRUBB, OP_SPLIT, Table, _SHAPES, _bases,  # noqa: F401
                              _pool, _regions, _token, cut_pairs, host_loop)

WIDTH = 80                   # bases per line of the output (noodles::fasta::Writer; host/editors.cc: write_fasta)
_SEP = re.compile(rb"[ \t\x0c]")  # what ends a name (host/editors.cc: is_ws, without the line ends)


def wrap(seq):
    return b"".join(seq[i:i + WIDTH] + b"\n" for i in range(0, len(seq), WIDTH))


def _records(text):
    """-> [(header line without '>', sequence)]; ValueError on a non-blank line in front of the first header"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()  # (a last line without its newline is a line)
    recs = []
    for l in lines:
        if l.startswith(b">"):
            recs.append([l[1:], []])
        elif recs:
            recs[-1][1].append(l)
        elif l:
            raise ValueError("Reading of the file in fasta format failed")
    return [(h, b"".join(s)) for h, s in recs]


def _split_header(head):
    m = _SEP.search(head)
    return (head, b"") if m is None else (head[:m.start()], head[m.end():])


def _verdict(op, table, name):
    regions, length, rtype = table.get(name)  # the key is the whole name
    if op == OP_FILTER:
        what = "copy" if rtype == NOT_BAD else "drop"
    elif op == OP_EXTRACT:
        what = "copy" if rtype != NOT_BAD else "drop"
    elif rtype == NOT_COVERED:
        what = "drop"
    elif (not regions) if op == OP_SCRUBB else rtype == NOT_BAD:
        what = "copy"
    else:
        what = "cut"
    return what, regions, length


def restate(text, op, table):
    """the four editors over a CR-free FASTA text -> (output bytes, records in, records out)"""
    out = []
    recs = _records(text)
    for head, seq in recs:
        name, desc = _split_header(head)
        what, regions, length = _verdict(op, table, name)
        if what == "copy":
            out.append(b">" + name + (b" " + desc if desc else b"") + b"\n" + wrap(seq))
        elif what == "cut":
            for p0, p1 in cut_pairs(op, regions, length):
                if p0 > len(seq) or p1 > len(seq):
                    break  # (the host's [ERROR] line: this position and the next are ignored)
                if p0 > p1:
                    raise ValueError("bad region with begin > end")
                out.append(b">" + name + b"_%d_%d\n" % (p0, p1) + wrap(seq[p0:p1]))
    return b"".join(out), len(recs), len(out)


def device_takes(text, table, op):
    """section "what falls back" of the interface, restated: True when the device editor takes `text` for `op`"""
    if not text:
        return True
    if b"\r" in text or not text.endswith(b"\n"):
        return False
    try:
        recs = _records(text)
    except ValueError:
        return False
    for head, seq in recs:
        name, _ = _split_header(head)
        if not name:
            return False
        what, regions, length = _verdict(op, table, name)
        if what == "cut":
            for p0, p1 in cut_pairs(op, regions, length):
                if p0 > len(seq) or p1 > len(seq) or p0 > p1:
                    return False
    return True


# ---- the generator ---------------------------------------------------------------------------------------------------------
_LENGTHS = [0, 1, 79, 80, 81, 159, 160, 161, 200, 1000]
_WIDTHS = [1, 7, 60, 70, 80, 81, None, "ragged"]  # None: the sequence on one line


def lay_out(rng, seq, width, blanks=0.0):
    """the sequence's lines as the input has them: of `width` bases, on one line, or ragged (0 to 90 bases a line, so blank
    lines too); `blanks`: the chance of a blank line behind any line"""
    if width is None:
        lines = [seq] if seq else []
    elif width == "ragged":
        lines, i = [], 0
        while i < len(seq):
            k = rng.randint(0, 90)
            lines.append(seq[i:i + k])
            i += k
    else:
        lines = [seq[i:i + width] for i in range(0, len(seq), width)]
    out = []
    for l in lines:
        out.append(l + b"\n")
        if blanks and rng.random() < blanks:
            out.append(b"\n" * rng.randint(1, 3))
    return b"".join(out)


def _case(rng, lengths_of, n_records, widths=_WIDTHS):
    ids = _pool(rng)
    names, lens, regs, types = [], [], [], []
    for i in ids:
        if rng.random() < 1 / 3:
            continue  # absent from the table
        length = lengths_of()
        names.append(i), lens.append(length), regs.append(_regions(rng, rng.choice(_SHAPES), length)), types.append(rng.randint(0, 2))
    table = Table(names, lens, regs, types)
    parts = [b"\n" * rng.randint(1, 3)] if rng.random() < 0.2 else []  # blank lines in front of the first header
    for _ in range(n_records):
        key = rng.choice(ids)
        _, length, _ = table.get(key)
        n = length if key in table.by_key else lengths_of()
        if key in table.by_key and rng.random() < 0.2:
            n += rng.randint(1, 9)  # a sequence longer than the table says: every position still lies inside it
        head = b">" + key
        u = rng.random()
        if u < 0.15:
            head += rng.choice([b" ", b"\t", b"\x0c"])  # an empty description behind its separator
        elif u < 0.6:
            head += rng.choice([b" ", b"\t", b"\x0c"]) + _token(rng, rng.randint(1, 40))
            if rng.random() < 0.4:
                head += rng.choice([b" x", b"\ty", b"  >z ", b" \x0c", b"\t"])  # more whitespace, a '>', a trailing blank
        width = rng.choice(widths)
        parts.append(head + b"\n" + lay_out(rng, _bases(rng, n), width, blanks=0.15 if rng.random() < 0.3 else 0.0))
        if rng.random() < 0.15:
            parts.append(b"\n" * rng.randint(1, 2))  # blank lines behind a record
    return b"".join(parts), table


def fuzz_cases(n_small=150, seed=20241203):
    """(tag, text, Table) — every text is one the device takes for all four ops"""
    rng = random.Random(seed)
    for k in range(n_small):
        yield ("small%d" % k,) + _case(rng, lambda: rng.choice(_LENGTHS), rng.randint(1, 12))
    for k in range(4):  # 4- and 5-digit positions, records of many lines
        yield ("mid%d" % k,) + _case(rng, lambda: rng.choice([10000, 12345, 65536, 99999, 100000]), 5, widths=[7, 60, 80, 81, None, "ragged"])
    yield ("digits7",) + _case(rng, lambda: 1200000, 2, widths=[80, None])
    yield "empty", b"", Table()
    yield "blank_lines_only", b"\n\n\n", Table()
    yield "empty_table", b">r\nACGT\n>r d\n>q\n\n", Table()
    yield "whole_body_one_region", b">r\nACGT\n", Table([b"r"], [4], [[(0, 4)]], [CHIMERIC])


_GOOD = b">ok a b\nACGTAC\nGTAC\n"


def fallback_cases():
    """(tag, ops, text, Table): `text` behind any run of good records must fall back for every op of `ops`.  Every text begins
    with a good record, so what stands behind the prefix is never in front of the first header — but "bases_first", which is
    tried alone."""
    t = Table([b"ok", b"far", b"rev"], [10, 40, 10], [[(2, 4)], [(20, 30)], [(2, 8), (5, 9)]], [CHIMERIC, CHIMERIC, CHIMERIC])
    cut = (OP_SCRUBB, OP_SPLIT)
    return [
        ("crlf", OPS, _GOOD + _GOOD.replace(b"\n", b"\r\n") + _GOOD, t),
        ("lone_cr", OPS, _GOOD + b">ok\nACGT\rACGTAC\n", t),
        ("no_final_newline", OPS, _GOOD + _GOOD[:-1], t),
        ("no_final_newline_header", OPS, _GOOD + b">ok", t),
        ("bare_mark", OPS, _GOOD + b">\nACGT\n" + _GOOD, t),
        ("no_name", OPS, _GOOD + b"> desc\nACGT\n" + _GOOD, t),
        ("no_name_tab", OPS, _GOOD + b">\tdesc\nACGT\n", t),
        ("position_beyond_read", cut, _GOOD + b">far\nACGTACGT\nACGT\n" + _GOOD, t),
        ("begin_after_end", cut, _GOOD + b">rev\nACGTACGTAC\n" + _GOOD, t),
    ]


BASES_FIRST = [b"ACGT\n" + _GOOD, b"\n\nA\n" + _GOOD, b" \n" + _GOOD]  # a non-blank line in front of the first header
