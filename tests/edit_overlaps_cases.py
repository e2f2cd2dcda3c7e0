"""What tests/test_edit_overlaps.py (CPU) and tests/test_gpu_edit_overlaps.py (GPU) share: the rule of filter / extract on
an overlap file restated in ten lines, the seeded fuzz generator, and the host loop as the yardstick for bytes."""
import os
import random

import numpy as np

from yacrd_amd import host

TILE = 32768             # bytes of text per workgroup (csrc/gpu_text.h: kGpTile)
CHUNK = 4 << 20          # what one copy moves (csrc/gpu_text.h: kTextChunk)
OP_FILTER, OP_EXTRACT = 1, 2


def restate(text, op, table, m4):
    """filter.rs:140-228 / extract.rs:144-232 over bytes: split on the delimiter, fields 0 and ib, unknown -> NotBad,
    empty lines dropped, one newline per kept line.  -> (kept bytes, non-empty lines, kept lines)"""
    delim, ib = (b" ", 1) if m4 else (b"\t", 5)
    out, n_lines = [], 0
    for l in text.split(b"\n"):
        if not l:
            continue
        f = l.split(delim)
        n_lines += 1
        both_good = table.get(f[0], 0) == 0 and table.get(f[ib], 0) == 0
        if both_good == (op == OP_FILTER):
            out.append(l + b"\n")
    return b"".join(out), n_lines, len(out)


def host_loop(tmp, op, text, names, types, ext):
    """yacrd_edit_file (the parent's one-thread loop) on `text` written to a file of extension `ext` -> its output bytes"""
    src, out = os.path.join(tmp, "h_in" + ext), os.path.join(tmp, "h_out" + ext)
    with open(src, "wb") as f:
        f.write(text)
    R = len(names)
    host.edit_file(op, src, out, [n.decode() for n in names], np.ones(R, np.uint32), np.zeros(R + 1, np.uint64),
                   np.zeros((0, 2), np.uint32), np.asarray(types, np.uint8), n_threads=1)
    with open(out, "rb") as f:
        return f.read()


_ALPHA = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_/.:-|"


def _token(rng, n):
    return bytes(rng.choice(_ALPHA) for _ in range(n))


def _pool(rng):
    """ids of 1 to 300 bytes, some of them prefixes of one another; a third is absent from the table"""
    ids = set()
    while len(ids) < rng.randint(2, 12):
        n = rng.choice([1, 1, 2, 3, 5, 8, 13, 21, 40, 80, 150, 299, 300])
        x = _token(rng, n)
        ids.add(x)
        if rng.random() < 0.5 and n > 1:
            ids.add(x[:rng.randint(1, n - 1)])  # a prefix
        if rng.random() < 0.3 and n < 300:
            ids.add(x + _token(rng, rng.randint(1, 300 - n)))  # an extension
    ids = sorted(ids)
    rng.shuffle(ids)
    n_absent = len(ids) // 3
    known = ids[n_absent:]
    types = [rng.choice([0, 0, 1, 2]) for _ in known]
    return ids, known, types


def _line(rng, ids, cols, m4, tail=0):
    delim, ib = (b" ", 1) if m4 else (b"\t", 5)
    f = [_token(rng, rng.randint(0, 6)) for _ in range(cols)]  # (an empty column is a column)
    f[0], f[ib] = rng.choice(ids), rng.choice(ids)
    if tail:
        f[-1] = f[-1] + _token(rng, 1) * tail
    return delim.join(f)


def _sized(rng, ids, cols, m4, size):
    """a text of exactly `size` bytes: lines until it is nearly full, the last one's last column stretched to fit"""
    parts, have = [], 0
    while True:
        l = _line(rng, ids, cols, m4) + b"\n"
        if have + len(l) + 700 > size:
            break
        parts.append(l)
        have += len(l)
        if rng.random() < 0.05 and have + 701 < size:
            parts.append(b"\n")
            have += 1
    last = _line(rng, ids, cols, m4)
    pad = size - have - len(last) - 1
    assert pad >= 0
    parts.append(last + b"x" * pad + b"\n")
    text = b"".join(parts)
    assert len(text) == size
    return text


def fuzz_cases(n_small=1000, seed=20241108):
    """-> (tag, text, m4, names, types) — `n_small` small texts and the shaped ones: 0 and 1 line, empty lines, no final
    newline, a line longer than a tile, sizes around 1, 2 and 3 tiles and around one 4 MiB chunk; PAF and M4 twins."""
    rng = random.Random(seed)
    for i in range(n_small):
        m4 = bool(i & 1)
        ids, known, types = _pool(rng)
        cols = rng.randint(9, 17)
        n_lines = rng.choice([0, 1, 1, 2, 3, 5, 8, 20, 40])
        parts = []
        for _ in range(n_lines):
            while rng.random() < 0.15:
                parts.append(b"")
            parts.append(_line(rng, ids, cols, m4))
        while rng.random() < 0.2:
            parts.append(b"")
        text = b"\n".join(parts)
        if parts and rng.random() < 0.7:
            text += b"\n"
        yield "small%d" % i, text, m4, known, types
    for m4 in (False, True):
        ids, known, types = _pool(rng)
        cols = rng.randint(9, 17)
        yield "empty", b"", m4, known, types
        yield "newlines", b"\n\n\n", m4, known, types
        yield "one", _line(rng, ids, cols, m4) + b"\n", m4, known, types
        yield "one_open", _line(rng, ids, cols, m4), m4, known, types
        # a line longer than one tile (and than two), between ordinary ones, with and without a final newline
        for tail in (TILE + 1200, 2 * TILE + 77, 5 * TILE):
            for open_end in (False, True):
                lines = [_line(rng, ids, cols, m4) for _ in range(3)] + [_line(rng, ids, cols, m4, tail=tail)] + \
                        [_line(rng, ids, cols, m4) for _ in range(2)]
                if open_end:
                    lines.append(_line(rng, ids, cols, m4, tail=tail))
                yield "long%d%s" % (tail, "_open" if open_end else ""), b"\n".join(lines) + (b"" if open_end else b"\n"), m4, known, types
        for k in (1, 2, 3):
            for d in (-17, -1, 0, 1, 16):
                text = _sized(rng, ids, cols, m4, k * TILE + d)
                yield "tile%d%+d" % (k, d), text, m4, known, types
                yield "tile%d%+d_open" % (k, d), text[:-1], m4, known, types
        for d in (-1, 0, 1):
            text = _sized(rng, ids, cols, m4, CHUNK + d)
            yield "chunk%+d" % d, text, m4, known, types
        yield "chunk+0_open", _sized(rng, ids, cols, m4, CHUNK + 1)[:-1], m4, known, types
