"""What tests/test_report_write_cases.py (CPU) and tests/test_gpu_report_write.py (GPU) share: the `.yacrd` report's format
(src/editor/mod.rs:61-107; host/report.cc: yacrd_report_write) restated in a few lines, the host writer through ctypes as
the yardstick (names as BYTES: an id is any bytes), a seeded maker of tables and the edge table."""
import ctypes
import os
from collections import namedtuple

import numpy as np

import report_cases as rc
from yacrd_amd import host

TYPE = (b"NotBad", b"Chimeric", b"NotCovered")
U32 = 0xFFFFFFFF
Table = namedtuple("Table", "names lengths bad_offsets bad_regions read_type")  # bytes ids, u32, u64[R + 1], u32[G, 2], u8


def restate(t):
    """The writer's rule: a Table -> the report's bytes."""
    out = []
    for r, (name, length) in enumerate(zip(t.names, t.lengths)):
        regs = t.bad_regions[int(t.bad_offsets[r]):int(t.bad_offsets[r + 1])]
        pieces = [b"%d,%d,%d" % ((int(e) - int(b)) & U32, b, e) for b, e in regs]  # end - begin as u32, wrapping
        out.append(TYPE[t.read_type[r]] + b"\t" + name + b"\t%d\t" % length + b";".join(pieces) + b"\n")
    return b"".join(out)


def table(names, lengths, regions_per_read, types):
    """names [bytes], lengths, a list of (begin, end) lists, types -> a Table"""
    bo = np.zeros(len(names) + 1, np.uint64)
    if names:
        np.cumsum([len(x) for x in regions_per_read], out=bo[1:])
    br = np.array([p for x in regions_per_read for p in x], np.uint32).reshape(-1, 2)
    return Table(list(names), np.array(lengths, np.uint32), bo, br, np.array(types, np.uint8))


def host_write(path, t):
    """yacrd_report_write on the table's arrays -> the bytes of the file it wrote; raises host.HostError"""
    lib = host.load_library()
    u64p, u32p, u8p = (ctypes.POINTER(c) for c in (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint8))
    R = len(t.names)
    off = np.zeros(R + 1, np.uint64)
    if R:
        np.cumsum([len(n) for n in t.names], out=off[1:])
    blob = ctypes.create_string_buffer(b"".join(t.names), int(off[-1]) + 1)
    lens = np.ascontiguousarray(t.lengths, np.uint32) if R else np.zeros(1, np.uint32)
    bo = np.ascontiguousarray(t.bad_offsets, np.uint64)
    br = np.ascontiguousarray(t.bad_regions, np.uint32).reshape(-1)
    if br.size == 0:
        br = np.zeros(2, np.uint32)
    rt = np.ascontiguousarray(t.read_type, np.uint8) if R else np.zeros(1, np.uint8)
    view = host._View(R, 0, 0, None, None, lens.ctypes.data_as(u32p), off.ctypes.data_as(u64p),
                      ctypes.cast(blob, ctypes.POINTER(ctypes.c_char)))
    host._check(lib, lib.yacrd_report_write(os.fsencode(path), ctypes.byref(view), bo.ctypes.data_as(u64p), br.ctypes.data_as(u32p),
                                            rt.ctypes.data_as(u8p)))
    with open(path, "rb") as f:
        return f.read()


def make_table(seed, tmp):
    """A seeded table: what the host reader makes of report_cases.make_text(seed) — ids of any bytes but tab and newline,
    the empty one among them, 0 to 40 regions per read, values at the ends of u32 —, the types cycling through 0 / 1 / 2."""
    names, lengths, bo, br = rc.host_read(tmp, rc.make_text(seed), "w_in.yacrd")
    types = (np.arange(len(names)) + seed) % 3
    return Table(names, lengths, bo, br.reshape(-1, 2), types.astype(np.uint8))


# ---- the edge table: one read per case -----------------------------------------------------------------------------------
EDGE_VALUES = sorted({0, U32} | {10 ** k - 1 for k in range(1, 10)} | {10 ** k for k in range(1, 10)})  # 0, 9, 10, 99, 100 ... 10^9 - 1, 10^9, 2^32 - 1


def edge_table():
    names, lengths, regs = [], [], []

    def add(name, length, regions):
        names.append(name), lengths.append(length), regs.append(regions)
    for i, v in enumerate(EDGE_VALUES):
        add(b"len-%d" % i, v, [])
        add(b"begin-%d" % i, 7, [(v, U32)])
        add(b"end-%d" % i, 7, [(0, v), (v, v)])
    add(b"wraps", 1000, [(500, 20), (U32, 0), (1, 0)])  # end < begin: the difference wraps in u32
    add(b"", 5, [(1, 2)])  # an empty id
    add(b"x", 5, [])
    add(b"y" * 255, 5, [(3, 4)])
    add((bytes(range(11, 256)) * 286)[:70000], 5, [(5, 6), (7, 8)])  # 70 000 bytes, none of them a tab or a newline
    add(b"a\rb;c,d e", 5, [(9, 10)])
    add(b"no-region", 123456, [])
    return table(names, lengths, regs, [i % 3 for i in range(len(names))])
