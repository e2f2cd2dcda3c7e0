"""What tests/test_report_cases.py (CPU) and tests/test_gpu_report.py (GPU) share: the rule of the `.yacrd` re-reader
(FromReport, src/stack.rs:176-257; host/editors.cc: yacrd_report_read) restated in a few lines, the seeded maker of report
texts, the corrupt cases, and the host reader through ctypes as the yardstick (names as BYTES: an id is any bytes)."""
import ctypes
import os
import random

import numpy as np

from yacrd_amd import host

TILE = 32768             # bytes of text per workgroup of the count / parse kernels (csrc/gpu_text.h: kGpTile)
CHUNK = 4 << 20          # what one copy moves (csrc/gpu_text.h: kTextChunk)
U32 = 0xFFFFFFFF


class Corrupt(Exception):
    pass


def _num(s):
    if not s or not s.isdigit() or int(s) > U32:  # (bytes.isdigit: ASCII digits only)
        raise Corrupt(s)
    return int(s)


def restate(text):
    """The reader's rule over bytes -> (names [bytes], lengths u32, bad_offsets u64, bad_regions u32[G, 2])."""
    rows = {}  # id -> (len, regions); assigning to a key that exists keeps its position: the last line wins, the first places
    for l in text.split(b"\n"):
        l = l[:-1] if l.endswith(b"\r") else l
        if not l:
            continue
        f = l.split(b"\t", 3)  # the type (ignored), the id, the length, the body with whatever tabs it holds
        if len(f) < 4:
            raise Corrupt(l)
        regs = []
        for piece in (f[3].split(b";") if f[3] else []):
            c = piece.split(b",")  # c[0] is never looked at, nor is anything behind a third comma
            if len(c) < 3:
                raise Corrupt(piece)
            regs.append((_num(c[1]), _num(c[2])))
        rows[f[1]] = (_num(f[2]), regs)
    names = list(rows)
    lengths = np.array([rows[k][0] for k in names], np.uint32)
    bo = np.zeros(len(names) + 1, np.uint64)
    np.cumsum([len(rows[k][1]) for k in names], out=bo[1:])
    br = np.array([r for k in names for r in rows[k][1]], np.uint32).reshape(-1, 2)
    return names, lengths, bo, br


def host_read_file(path):
    """yacrd_report_read + yacrd_report_get -> the same tuple as restate; raises host.HostError on a corrupt report."""
    lib = host.load_library()
    h = ctypes.c_void_p()
    host._check(lib, lib.yacrd_report_read(os.fsencode(path), ctypes.byref(h)))
    try:
        v = host._BadParts()
        host._check(lib, lib.yacrd_report_get(h, ctypes.byref(v)))
        R = int(v.n_reads)
        off = np.ctypeslib.as_array(v.name_off, shape=(R + 1,)).copy()
        blob = ctypes.string_at(v.names, int(off[-1])) if R else b""
        names = [blob[int(off[i]):int(off[i + 1])] for i in range(R)]
        lengths = np.ctypeslib.as_array(v.lengths, shape=(R,)).copy() if R else np.zeros(0, np.uint32)
        bo = np.ctypeslib.as_array(v.bad_offsets, shape=(R + 1,)).copy()
        G = int(bo[-1])
        br = (np.ctypeslib.as_array(v.bad_regions, shape=(2 * G,)).copy().reshape(-1, 2) if G else np.zeros((0, 2), np.uint32))
    finally:
        lib.yacrd_report_free(h)
    return names, lengths, bo, br


def host_read(tmp, text, name="h_in.yacrd"):
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(text)
    return host_read_file(path)


def same(a, b):
    """two (names, lengths, bad_offsets, bad_regions) tuples, bit for bit"""
    return (list(a[0]) == list(b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and
            np.array_equal(np.asarray(a[3]).reshape(-1, 2), np.asarray(b[3]).reshape(-1, 2)))


# ---- the maker ----------------------------------------------------------------------------------------------------------
_ID_BYTES = bytes(b for b in range(1, 256) if b not in (9, 10))  # an id: anything but a tab and a newline (CR, ';', ',' included)
_PLAIN = b"ACGTacgt0123456789_/:.-"


def _garbage(rng, lo, hi, forbid):
    n = rng.randint(lo, hi)
    return bytes(b for b in rng.choices(range(256), k=n) if b not in forbid and b != 10)


def _value(rng):
    return rng.choice([0, 1, U32, U32 - 1, rng.randint(0, 70000), rng.randint(0, U32)])


def _row(rng, rid, n_reg, eol):
    col1 = rng.choice([b"NotBad", b"Chimeric", b"NotCovered", b"", _garbage(rng, 0, 12, (9,))])
    pieces = []
    for _ in range(n_reg):
        first = rng.choice([b"%d" % _value(rng), b"", _garbage(rng, 0, 6, (ord(","), ord(";")))])
        p = first + b",%d,%d" % (_value(rng), _value(rng))
        if rng.random() < 0.15:
            p += b"," + _garbage(rng, 0, 8, (ord(";"),))  # a fourth field: ignored, commas and tabs and all
        pieces.append(p)
    lead = b"0" * rng.choice([0, 0, 0, 3])  # leading zeros are digits
    return col1 + b"\t" + rid + b"\t" + lead + b"%d" % _value(rng) + b"\t" + b";".join(pieces) + eol


def make_text(seed, size=None):
    """A report the rule accepts.  size: None = a few KB at most; else EXACTLY that many bytes (>= 64), reached by a last
    row whose first column is as long as it takes."""
    rng = random.Random(seed)
    crlf = rng.random() < 0.3
    eol = lambda: b"\r\n" if (crlf and rng.random() < 0.9) else b"\n"
    budget = size - 40 if size is not None else rng.choice([0, 60, 400, 3000, 6000])
    repeat = 1
    if size is not None and size > 8 * TILE:  # a large text is a block of ~128 KiB, repeated
        repeat = size // (4 * TILE)
        budget = budget // repeat
    ids, out, total = [], [], 0
    max_id = 300 if size is None or size < 3 * TILE + 64 else 40
    while total < budget:
        r = rng.random()
        if ids and r < 0.08:
            base = rng.choice(ids)
            rid = base[:rng.randint(0, len(base))]  # a prefix of another id (the empty id is legal)
        elif r < 0.6:
            rid = bytes(rng.choices(_PLAIN, k=rng.randint(1, 24)))
        else:
            rid = bytes(rng.choices(_ID_BYTES, k=rng.randint(0, max_id)))
        ids.append(rid)
        reps = rng.randint(2, 4) if rng.random() < 0.10 else 1
        rows = []
        for k in range(reps):
            n_reg = rng.choice([0, 0, 1, 1, 2, 3, rng.randint(0, 40)])
            if reps > 1 and k == reps - 1 and rng.random() < 0.4:
                n_reg = 0  # a repeat whose last row has an empty body
            rows.append(_row(rng, rid, n_reg, eol()))
        for row in rows:
            if size is not None and total + len(row) > budget:
                total = budget
                break
            # a repeat lands somewhere behind its first row, not always next to it
            out.insert(rng.randint(max(0, len(out) - 30), len(out)) if row is not rows[0] and out else len(out), row)
            total += len(row)
            if rng.random() < 0.05:
                blank = rng.choice([b"\n", b"\r\n"])
                if size is None or total + len(blank) <= budget:
                    out.append(blank)
                    total += len(blank)
    text = b"".join(out)
    if repeat > 1:
        text = text * repeat  # every id again and again: each line but the last of its id is replaced
    if size is not None:
        tail = b"\tlast-row\t7\t1,2,3"
        final_nl = b"" if rng.random() < 0.5 else b"\n"
        text += b"x" * (size - len(text) - len(tail) - len(final_nl)) + tail + final_nl
        assert len(text) == size
    elif text and rng.random() < 0.3:
        text = text.rstrip(b"\r\n")  # no final newline
        if text.endswith(b"\t") or not text:
            text += b"\n"  # (stripping must not eat into an empty body's line end only: keep it a line)
    return text


def fuzz_sizes(seed):
    """every 10th text sits on a border of 1 / 2 / 3 tiles, every 60th on the chunk border; the rest are small"""
    if seed % 60 == 59:
        return CHUNK + (-1, 0, 1, 77)[(seed // 60) % 4]
    if seed % 10 == 9:
        return (1 + (seed // 10) % 3) * TILE + (-1, 0, 1, 2, 130, -129)[(seed // 30) % 6]
    return None


# ---- what the reader calls corrupt ----------------------------------------------------------------------------------------
GOOD_ROW = b"NotBad\tread-ok\t1000\t12,0,12;5,995,1000\n"
CORRUPT = {
    "two_columns": b"Chimeric\tread-a\n",
    "len_12a": b"NotBad\tread-a\t12a\t\n",
    "len_2_32": b"NotBad\tread-a\t4294967296\t\n",
    "one_comma": b"NotBad\tread-a\t100\t5,7\n",
    "trailing_semicolon": b"NotBad\tread-a\t100\t5,0,5;\n",
    "empty_begin": b"NotBad\tread-a\t100\t5,,5\n",
}


def corrupt_text(name, rows_before=3, rows_after=2):
    return GOOD_ROW * rows_before + CORRUPT[name] + GOOD_ROW * rows_after
