"""What tests/test_edit_fastq_cases.py (CPU) and tests/test_gpu_edit_fastq.py (GPU) share: which FASTQ texts the device editor
takes (include/yacrd_engine.h: yacrd_engine_edit_fastq), the four editors' rules restated over canonical records, the seeded
case generator, the set of texts that must fall back, and the host loop as the yardstick for bytes."""
import os
import random
import re

import numpy as np

from yacrd_amd import host

TILE = 32768                 # bytes of text per workgroup (csrc/gpu_text.h: kGpTile)
SEGMENT = 32 * (4 << 20)     # what the mover hands on at once (csrc/gpu_text.h: kTextChunk * kTextSeg)
OUT_TILE = 4096              # bytes of output per workgroup of the copy pass (csrc/gpu_seq_edit.hip: kSqOutTile)
OP_SCRUBB, OP_FILTER, OP_EXTRACT, OP_SPLIT = 0, 1, 2, 3
OPS = (OP_SCRUBB, OP_FILTER, OP_EXTRACT, OP_SPLIT)
OP_NAMES = {OP_SCRUBB: "scrubb", OP_FILTER: "filter", OP_EXTRACT: "extract", OP_SPLIT: "split"}
NOT_BAD, CHIMERIC, NOT_COVERED = 0, 1, 2

_WS = re.compile(rb"[ \t\n\x0c\r]")  # host/editors.cc: is_ws


class Table:
    """the bad-part table of a case: ids (bytes), lengths, regions per read, types"""

    def __init__(self, names=(), lengths=(), regions=(), types=()):
        self.names, self.lengths, self.regions, self.types = list(names), list(lengths), [list(r) for r in regions], list(types)
        self.by_key = {n: (self.regions[i], self.lengths[i], self.types[i]) for i, n in enumerate(self.names)}

    def get(self, key):
        return self.by_key.get(key, ([], 0, NOT_BAD))  # an id the table does not hold is NotBad with no region

    def arrays(self):
        """-> (names as str, lengths u32, bad_offsets u64[R + 1], bad_regions u32[G, 2], read_type u8)"""
        off = np.zeros(len(self.names) + 1, np.uint64)
        if self.names:
            off[1:] = np.cumsum([len(r) for r in self.regions], dtype=np.uint64)
        flat = [p for r in self.regions for p in r]
        return ([n.decode() for n in self.names], np.array(self.lengths, np.uint32), off,
                np.array(flat, np.uint32).reshape(-1, 2), np.array(self.types, np.uint8))


def cut_pairs(op, regions, length):
    """cut_positions and the loop behind it (host/editors.cc; scrubbing.rs:195-209, split.rs:189-198)"""
    poss = [0]
    if op == OP_SCRUBB:
        for b, e in regions:
            poss += [b, e]
        if poss[-1] != length:
            poss.append(length)
        first = 2 if len(poss) >= 2 and poss[0] == 0 and poss[1] == 0 else 0
    else:
        for b, e in regions:
            if b == 0 or e == length:
                continue
            poss += [b, e]
        poss.append(length)
        first = 0
    return [(poss[k], poss[k + 1]) for k in range(first, len(poss) - 1, 2)]  # a trailing odd element is ignored


def _records(text):
    lines = text.split(b"\n")
    return [lines[i:i + 4] for i in range(0, len(lines) - 1, 4)]


def _verdict(op, table, head):
    """-> ("drop" | "copy" | "cut", name, desc, regions, length) for the header line without its '@'"""
    name, _, desc = head.partition(b" ")
    regions, length, rtype = table.get(_WS.split(name)[0])
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
    return what, name, desc, regions, length


def device_takes(text, table, op):
    """section "what falls back" of the interface, restated: True when the device editor takes `text` for `op`"""
    if not text:
        return True
    if not text.endswith(b"\n") or b"\r" in text or text.count(b"\n") % 4:
        return False
    for head, seq, plus, qual in _records(text):
        if not head.startswith(b"@") or len(head) < 2 or head[1:2] == b" " or head.endswith(b" "):
            return False  # no '@', no name, "@name \n"
        if plus != b"+" or len(seq) != len(qual):
            return False
        what, _, _, regions, length = _verdict(op, table, head[1:])
        if what == "cut":
            for p0, p1 in cut_pairs(op, regions, length):
                if p0 > len(seq) or p1 > len(seq) or p0 > p1:
                    return False
    return True


def restate(text, op, table):
    """the four editors over a text the device takes -> (output bytes, records in, records out)"""
    out, n_in = [], 0
    for head, seq, _, qual in _records(text):
        n_in += 1
        what, name, desc, regions, length = _verdict(op, table, head[1:])
        if what == "copy":
            out.append(head + b"\n" + seq + b"\n+\n" + qual + b"\n")
        elif what == "cut":
            for p0, p1 in cut_pairs(op, regions, length):
                out.append(b"@" + name + b"_%d_%d" % (p0, p1) + (b" " + desc if desc else b"") + b"\n" + seq[p0:p1] + b"\n+\n" + qual[p0:p1] + b"\n")
    return b"".join(out), n_in, len(out)


def host_loop(tmp, op, text, table, ext=".fastq", n_threads=1):
    """yacrd_edit_file on `text` written to a file -> its output bytes"""
    src, out = os.path.join(tmp, "h_in" + ext), os.path.join(tmp, "h_out" + ext)
    with open(src, "wb") as f:
        f.write(text)
    if os.path.exists(out):
        os.remove(out)
    names, lengths, bo, br, rt = table.arrays()
    host.edit_file(op, src, out, names, lengths, bo, br, rt, n_threads=n_threads)
    with open(out, "rb") as f:
        return f.read()


def oracle_table(table):
    """the table as oracle/editors.py takes it, or None where the oracle does not apply: it derives every type from the
    regions (type_of_read at 0.4), so a case whose types are set freely is not its case"""
    import oracle
    for regions, length, rtype in table.by_key.values():
        if oracle.type_of_read(length, regions, 0.4) != rtype:
            return None
    return {n.decode(): (r, l) for n, (r, l, _) in table.by_key.items()}


# ---- the generator ---------------------------------------------------------------------------------------------------------
_ALPHA = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_/.:-|@+"


def _token(rng, n):
    return bytes(rng.choice(_ALPHA) for _ in range(n))


def _bases(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(rng.getrandbits(32)).integers(0, 4, n)]) if n > 64 \
        else bytes(rng.choice(b"ACGT") for _ in range(n))


def _quals(rng, n):
    if n > 64:
        return bytes(np.random.default_rng(rng.getrandbits(32)).integers(33, 127, n, dtype=np.uint8))
    q = bytearray(rng.randint(33, 126) for _ in range(n))
    if n and rng.random() < 0.3:
        q[0] = rng.choice(b"@+")  # a quality line that looks like a header or a separator
    return bytes(q)


def _pool(rng):
    """ids of 1 to 300 bytes, some of them prefixes of one another"""
    ids = set()
    while len(ids) < rng.randint(2, 10):
        n = rng.choice([1, 1, 2, 3, 5, 8, 13, 21, 40, 80, 150, 299, 300])
        x = _token(rng, n)
        ids.add(x)
        if rng.random() < 0.5 and n > 1:
            ids.add(x[:rng.randint(1, n - 1)])
        if rng.random() < 0.3 and n < 300:
            ids.add(x + _token(rng, rng.randint(1, 300 - n)))
    return sorted(ids)


_SHAPES = ("none", "from0", "to_len", "both_ends", "adjacent", "everything", "middle", "many")


def _regions(rng, shape, length):
    """sorted regions inside [0, length] of the named shape (fewer where the read is too short for it)"""
    if shape == "none" or length == 0:
        return []
    if shape == "everything":
        return [(0, length)]
    third = max(1, length // 3)
    if shape == "from0":
        return [(0, rng.randint(1, third))]
    if shape == "to_len":
        return [(length - rng.randint(1, third), length)]
    if shape == "both_ends":  # the read vanishes under scrubb when the two meet
        a = rng.randint(1, third)
        return [(0, a), (a if rng.random() < 0.5 else min(length, a + rng.randint(0, third)), length)]
    if shape == "adjacent":  # a zero-length piece, @id_5_5
        a = rng.randint(0, third)
        b = min(length, a + rng.randint(0, third))
        return [(a, b), (b, min(length, b + rng.randint(0, third)))]
    k = 1 if shape == "middle" else rng.randint(2, 9)
    cuts = sorted(rng.randint(0, length) for _ in range(2 * k))
    return [(cuts[2 * i], cuts[2 * i + 1]) for i in range(k)]


def _case(rng, lengths_of, n_records, consistent):
    """one text and its table; lengths_of(): a read's length; consistent: the types follow from the regions (the oracle's case)"""
    ids = _pool(rng)
    names, lens, regs, types = [], [], [], []
    for i in ids:
        if rng.random() < 1 / 3:
            continue  # absent from the table
        length = lengths_of()
        shape = rng.choice(_SHAPES)
        r = _regions(rng, shape, length)
        names.append(i), lens.append(length), regs.append(r)
        types.append(rng.randint(0, 2))
    table = Table(names, lens, regs, types)
    if consistent:
        import oracle
        table = Table(names, lens, regs, [oracle.type_of_read(l, r, 0.4) for l, r in zip(lens, regs)])
    recs = []
    for _ in range(n_records):
        key = rng.choice(ids)
        _, length, _ = table.get(key)
        n = length if key in table.by_key else lengths_of()
        if key in table.by_key and rng.random() < 0.2:
            n += rng.randint(1, 9)  # a sequence longer than the table says: every position still lies inside it
        name = key + (b"\t" + _token(rng, rng.randint(0, 5)) if rng.random() < 0.2 else b"")  # a tab: the key is shorter than the name
        desc = b" " + _token(rng, rng.randint(1, 40)) + (b" x" if rng.random() < 0.3 else b"") if rng.random() < 0.5 else b""
        rec = b"@" + name + desc + b"\n" + _bases(rng, n) + b"\n+\n" + _quals(rng, n) + b"\n"
        recs.append(rec)
        if rng.random() < 0.15:
            recs.append(rec)  # a duplicate record
    return b"".join(recs), table


def fuzz_cases(n_small=240, seed=20241119):
    """(tag, text, Table) — every text is one the device takes for all four ops"""
    rng = random.Random(seed)
    small = lambda: rng.choice([0, 1, 1, 2, 5, 9, 10, 11, 60, 99, 100, 101, 300, 999, 1000, 1001])
    for k in range(n_small):
        yield ("small%d" % k,) + _case(rng, small, rng.randint(1, 12), consistent=k % 2 == 0)
    for k in range(6):  # 4- and 5-digit positions; several tiles per line
        yield ("mid%d" % k,) + _case(rng, lambda: rng.choice([9999, 10000, 12345, 65535, 65536, 99999]), 6, consistent=k % 2 == 0)
    for k in range(2):
        yield ("long%d" % k,) + _case(rng, lambda: rng.choice([100000, 99999]), 4, consistent=k == 0)
    yield ("digits7",) + _case(rng, lambda: rng.choice([999999, 1000000, 1200000]), 3, consistent=False)  # 6- and 7-digit positions
    yield "empty", b"", Table()
    yield "empty_table", b"@r\nACGT\n+\n!!!!\n@r d\n\n+\n\n", Table()
    yield "whole_body_one_region", b"@r\nACGT\n+\n!!!!\n", Table([b"r"], [4], [[(0, 4)]], [CHIMERIC])


_GOOD = b"@ok a b\nACGTACGTAC\n+\n!!!!!!!!!!\n"


def fallback_cases():
    """(tag, ops, text, Table): `text` behind any run of good records must fall back for every op of `ops`"""
    t = Table([b"ok", b"far", b"rev"], [10, 40, 10], [[(2, 4)], [(20, 30)], [(2, 8), (5, 9)]], [CHIMERIC, CHIMERIC, CHIMERIC])
    cut = (OP_SCRUBB, OP_SPLIT)
    return [
        ("crlf", OPS, _GOOD + _GOOD.replace(b"\n", b"\r\n") + _GOOD, t),
        ("lone_cr", OPS, _GOOD + b"@ok\nACGT\rACGT\n+\n!!!!!!!!!\n", t),
        ("plus_name", OPS, _GOOD + b"@ok\nACGT\n+ok\n!!!!\n" + _GOOD, t),
        ("blank_line", OPS, _GOOD + b"\n" + _GOOD, t),
        ("four_blank_lines", OPS, _GOOD + b"\n\n\n\n" + _GOOD, t),
        ("no_final_newline", OPS, _GOOD + _GOOD[:-1], t),
        ("lengths_differ", OPS, _GOOD + b"@ok\nACGT\n+\n!!!\n" + _GOOD, t),
        ("bare_at", OPS, _GOOD + b"@\nACGT\n+\n!!!!\n", t),
        ("blank_before_newline", OPS, _GOOD + b"@ok \nACGT\n+\n!!!!\n", t),
        ("fifth_line", OPS, _GOOD + b"@ok\nACGT\n+\n!!!!\nACGT\n" + _GOOD, t),
        ("no_at", OPS, _GOOD + b"ok\nACGT\n+\n!!!!\n", t),
        ("position_beyond_read", cut, _GOOD + b"@far\nACGTACGTACGT\n+\n!!!!!!!!!!!!\n" + _GOOD, t),
        ("begin_after_end", cut, _GOOD + b"@rev\nACGTACGTAC\n+\n!!!!!!!!!!\n" + _GOOD, t),
    ]
