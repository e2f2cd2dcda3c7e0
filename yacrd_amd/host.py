"""ctypes binding of include/yacrd_host.h (libyacrd_host.so): ingest, report, synthetic data."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "lib", "libyacrd_host.so")

SYNTH_ONT, SYNTH_SEQUEL, SYNTH_SKEWED = 0, 1, 2
# yacrd_synth_cfg.flags (include/yacrd_host.h)
SYNTH_F_NO_INJECTION, SYNTH_F_JITTER, SYNTH_F_SIGMA_X4 = 1, 2, 4


def synth_f_chimera_pct(p):
    """YACRD_SYNTH_F_CHIMERA_PCT: per cent of the reads that are chimeras (default 2)."""
    return (int(p) & 0xFF) << 16


def synth_f_sigma(s):
    """sigma (positions) of the dovetail ends' offset (default 30): 1..255 exactly, up to 1020 in steps of 4
    (YACRD_SYNTH_F_SIGMA_X4)"""
    s = int(s)
    if not 0 <= s <= 1020:
        raise ValueError("sigma must be within 0..1020")
    return (SYNTH_F_SIGMA_X4 | ((s // 4) << 8)) if s > 255 else (s << 8)
FMT_AUTO, FMT_PAF, FMT_M4 = 0, 1, 2

EXPORTED_SYMBOLS = [
    "yacrd_host_last_error", "yacrd_csr_from_file", "yacrd_csr_from_memory", "yacrd_csr_get",
    "yacrd_csr_find", "yacrd_csr_free", "yacrd_report_write", "yacrd_synth_csr", "yacrd_synth_paf",
    "yacrd_edit_file", "yacrd_edit_file_mt", "yacrd_text_from_file", "yacrd_text_free", "yacrd_report_read", "yacrd_report_get", "yacrd_report_free",
    "yacrd_edit_file_to", "yacrd_file_compression", "yacrd_bgzf_encode_host", "yacrd_bgzf_decode_host", "yacrd_bytes_free", "yacrd_deflate_code_lengths",
    "yacrd_synth_fastq", "yacrd_ingest_stream", "yacrd_ingest_stream_memory", "yacrd_csr_handle_map", "yacrd_bgzf_plan_segments",
    "yacrd_bgzf_text_ends", "yacrd_bgzf_window_cuts", "yacrd_edit_window_route", "yacrd_gzip_stream_decode_host",
]

OP_SCRUBB, OP_FILTER, OP_EXTRACT, OP_SPLIT = 0, 1, 2, 3


class HostError(RuntimeError):
    pass


class _View(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_uint64), ("n_intervals", ctypes.c_uint64),
                ("n_records", ctypes.c_uint64),
                ("offsets", ctypes.POINTER(ctypes.c_uint64)),
                ("intervals", ctypes.POINTER(ctypes.c_uint32)),
                ("lengths", ctypes.POINTER(ctypes.c_uint32)),
                ("name_off", ctypes.POINTER(ctypes.c_uint64)),
                ("names", ctypes.POINTER(ctypes.c_char))]


class _Text(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("n", ctypes.c_uint64), ("cap", ctypes.c_uint64), ("members", ctypes.c_uint64),
                ("threads", ctypes.c_uint32), ("compression", ctypes.c_int32)]


class Text:
    """yacrd_text_from_file: a compressed (gzip / bzip2 / xz) file inflated into memory; .address / .n_bytes for
    Engine.ingest_text, .bytes() for a copy; None from text_from_file when the file is not compressed."""

    def __init__(self, lib, t):
        self._lib, self._t = lib, t
        self.address, self.n_bytes = int(t.data or 0), int(t.n)
        self.members, self.threads, self.compression = int(t.members), int(t.threads), int(t.compression)

    def bytes(self):
        return ctypes.string_at(self.address, self.n_bytes) if self.n_bytes else b""

    def close(self):
        if self._t is not None:
            self._lib.yacrd_text_free(ctypes.byref(self._t))
            self._t = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def text_from_file(path, n_threads=0):
    lib = load_library()
    t = _Text()
    rc = lib.yacrd_text_from_file(os.fsencode(path), n_threads, ctypes.byref(t))
    if rc == 2:
        return None
    _check(lib, rc)
    return Text(lib, t)


class _BadParts(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_uint64),
                ("name_off", ctypes.POINTER(ctypes.c_uint64)),
                ("names", ctypes.c_char_p),
                ("lengths", ctypes.POINTER(ctypes.c_uint32)),
                ("bad_offsets", ctypes.POINTER(ctypes.c_uint64)),
                ("bad_regions", ctypes.POINTER(ctypes.c_uint32)),
                ("read_type", ctypes.POINTER(ctypes.c_uint8))]


class _SynthCfg(ctypes.Structure):
    _fields_ = [("profile", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("n_reads", ctypes.c_uint64), ("n_overlaps", ctypes.c_uint64),
                ("seed", ctypes.c_uint64)]


_lib = None


def build(force=False):
    cmd = ["make", "-s", "-C", os.path.join(_HERE, "csrc", "host")]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return _LIB


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise HostError("%s is missing: run __graft_entry__.build()" % _LIB)
        lib = ctypes.CDLL(_LIB)
        lib.yacrd_host_last_error.restype = ctypes.c_char_p
        lib.yacrd_csr_from_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_void_p)]
        lib.yacrd_csr_from_memory.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int,
                                              ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        lib.yacrd_ingest_stream.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_void_p)]
        lib.yacrd_ingest_stream_memory.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.POINTER(ctypes.c_void_p)]
        lib.yacrd_csr_handle_map.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)),
                                             ctypes.POINTER(ctypes.c_uint64)]
        lib.yacrd_csr_get.argtypes = [ctypes.c_void_p, ctypes.POINTER(_View)]
        lib.yacrd_csr_find.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.yacrd_csr_find.restype = ctypes.c_int64
        lib.yacrd_csr_free.argtypes = [ctypes.c_void_p]
        lib.yacrd_csr_free.restype = None
        lib.yacrd_report_write.argtypes = [ctypes.c_char_p, ctypes.POINTER(_View),
                                           ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint8)]
        lib.yacrd_synth_csr.argtypes = [ctypes.POINTER(_SynthCfg), ctypes.POINTER(ctypes.c_uint64),
                                        ctypes.POINTER(ctypes.c_uint32),
                                        ctypes.POINTER(ctypes.c_uint32)]
        lib.yacrd_synth_paf.argtypes = [ctypes.POINTER(_SynthCfg), ctypes.c_char_p]
        lib.yacrd_synth_fastq.argtypes = [ctypes.POINTER(_SynthCfg), ctypes.c_uint64, ctypes.c_char_p]
        lib.yacrd_edit_file.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p,
                                        ctypes.POINTER(_BadParts)]
        lib.yacrd_text_from_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(_Text)]
        lib.yacrd_text_free.argtypes = [ctypes.POINTER(_Text)]
        lib.yacrd_text_free.restype = None
        lib.yacrd_edit_file_mt.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p,
                                           ctypes.POINTER(_BadParts), ctypes.c_int]
        lib.yacrd_edit_file_to.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(_BadParts), ctypes.c_int, ctypes.c_void_p]
        lib.yacrd_file_compression.argtypes = [ctypes.c_char_p]
        lib.yacrd_bgzf_encode_host.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        lib.yacrd_bgzf_decode_host.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        lib.yacrd_gzip_stream_decode_host.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p),
                                                      ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        lib.yacrd_bgzf_plan_segments.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                                 ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        lib.yacrd_bgzf_text_ends.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32),
                                             ctypes.POINTER(ctypes.c_int)]
        lib.yacrd_bgzf_window_cuts.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p),
                                               ctypes.POINTER(ctypes.c_uint64)]
        lib.yacrd_edit_window_route.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                                ctypes.POINTER(ctypes.c_uint64)]
        lib.yacrd_bytes_free.argtypes = [ctypes.c_void_p]
        lib.yacrd_bytes_free.restype = None
        lib.yacrd_deflate_code_lengths.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        lib.yacrd_report_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        lib.yacrd_report_get.argtypes = [ctypes.c_void_p, ctypes.POINTER(_BadParts)]
        lib.yacrd_report_free.argtypes = [ctypes.c_void_p]
        lib.yacrd_report_free.restype = None
        _lib = lib
    return _lib


def _check(lib, rc):
    if rc != 0:
        raise HostError(lib.yacrd_host_last_error().decode())


class Csr:
    """Owns a yacrd_csr; numpy views are copies so they outlive it."""

    def __init__(self, handle):
        self._lib = load_library()
        self._h = handle
        v = _View()
        _check(self._lib, self._lib.yacrd_csr_get(self._h, ctypes.byref(v)))
        self._view = v
        R, I = int(v.n_reads), int(v.n_intervals)
        self.n_reads, self.n_intervals, self.n_records = R, I, int(v.n_records)
        self.streamed = not bool(v.offsets)  # yacrd_ingest_stream: the CSR lives in HBM
        if self.streamed:
            self.offsets = self.intervals = None
            mp = ctypes.POINTER(ctypes.c_uint32)()
            nh = ctypes.c_uint64()
            _check(self._lib, self._lib.yacrd_csr_handle_map(self._h, ctypes.byref(mp), ctypes.byref(nh)))
            self.handle_map = (np.ctypeslib.as_array(mp, shape=(int(nh.value),)).copy()
                               if nh.value else np.zeros(0, np.uint32))
        else:
            self.offsets = np.ctypeslib.as_array(v.offsets, shape=(R + 1,)).copy()
            self.intervals = (np.ctypeslib.as_array(v.intervals, shape=(2 * I,)).copy().reshape(-1, 2)
                              if I else np.zeros((0, 2), np.uint32))
        self.lengths = (np.ctypeslib.as_array(v.lengths, shape=(R,)).copy()
                        if R else np.zeros(0, np.uint32))
        name_off = np.ctypeslib.as_array(v.name_off, shape=(R + 1,)).copy()
        blob = ctypes.string_at(v.names, int(name_off[-1])) if R else b""
        self.names = [blob[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(R)]

    def find(self, name):
        b = name.encode()
        return int(self._lib.yacrd_csr_find(self._h, b, len(b)))

    def write_report(self, path, bad_offsets, bad_regions, read_type):
        bo = np.ascontiguousarray(bad_offsets, dtype=np.uint64)
        br = np.ascontiguousarray(bad_regions, dtype=np.uint32).reshape(-1)
        if br.size == 0:
            br = np.zeros(2, np.uint32)
        rt = np.ascontiguousarray(read_type, dtype=np.uint8)
        if rt.size == 0:
            rt = np.zeros(1, np.uint8)
        _check(self._lib, self._lib.yacrd_report_write(
            path.encode(), ctypes.byref(self._view),
            bo.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            br.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            rt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))

    def close(self):
        if self._h:
            self._lib.yacrd_csr_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_from_file(path, fmt=FMT_AUTO, n_threads=0):
    lib = load_library()
    h = ctypes.c_void_p()
    _check(lib, lib.yacrd_csr_from_file(path.encode(), fmt, n_threads, ctypes.byref(h)))
    return Csr(h)


def ingest_stream(path, sink, fmt=FMT_AUTO, n_threads=0):
    """Parse `path`, handing the overlap records to `sink` (a yacrd_rec_sink struct, e.g.
    yacrd_amd.Stream.sink()) while parsing.  Returns a Csr with names / lengths / handle_map."""
    lib = load_library()
    h = ctypes.c_void_p()
    _check(lib, lib.yacrd_ingest_stream(path.encode(), fmt, n_threads, ctypes.addressof(sink), ctypes.byref(h)))
    return Csr(h)


def ingest_stream_memory(text, sink, fmt, n_threads=0):
    lib = load_library()
    if isinstance(text, str):
        text = text.encode()
    h = ctypes.c_void_p()
    _check(lib, lib.yacrd_ingest_stream_memory(text, len(text), fmt, n_threads, ctypes.addressof(sink),
                                               ctypes.byref(h)))
    return Csr(h)


def csr_from_memory(text, fmt, n_threads=0):
    lib = load_library()
    if isinstance(text, str):
        text = text.encode()
    h = ctypes.c_void_p()
    _check(lib, lib.yacrd_csr_from_memory(text, len(text), fmt, n_threads, ctypes.byref(h)))
    return Csr(h)


def synth_csr(profile, n_reads, n_overlaps, seed, flags=0):
    """Deterministic synthetic pile-up straight to CSR.
    Returns offsets u64[R+1], intervals u32[I,2], lengths u32[R]."""
    lib = load_library()
    cfg = _SynthCfg(profile, flags, n_reads, n_overlaps, seed)
    offsets = np.zeros(n_reads + 1, dtype=np.uint64)
    intervals = np.zeros(4 * n_overlaps, dtype=np.uint32)
    lengths = np.zeros(n_reads, dtype=np.uint32)
    _check(lib, lib.yacrd_synth_csr(ctypes.byref(cfg),
                                    offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                    intervals.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                    lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
    return offsets, intervals.reshape(-1, 2), lengths


def synth_paf(profile, n_reads, n_overlaps, seed, path, flags=0):
    lib = load_library()
    cfg = _SynthCfg(profile, flags, n_reads, n_overlaps, seed)
    _check(lib, lib.yacrd_synth_paf(ctypes.byref(cfg), path.encode()))


def synth_fastq(profile, n_reads, n_overlaps, seed, extra_reads, path, flags=0):
    lib = load_library()
    cfg = _SynthCfg(profile, flags, n_reads, n_overlaps, seed)
    _check(lib, lib.yacrd_synth_fastq(ctypes.byref(cfg), extra_reads, path.encode()))


class ByteSink(ctypes.Structure):
    """yacrd_byte_sink (both headers): somebody who takes bytes in order."""
    WRITE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)
    _fields_ = [("ctx", ctypes.c_void_p), ("write", WRITE)]


def _bad_parts(names, lengths, bad_offsets, bad_regions, read_type):
    """(the yacrd_badparts_view, what must stay alive while it is used)"""
    blob = b"".join(n.encode() for n in names)
    name_off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(n.encode()) for n in names], out=name_off[1:])
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    bo = np.ascontiguousarray(bad_offsets, dtype=np.uint64)
    br = np.ascontiguousarray(bad_regions, dtype=np.uint32).reshape(-1)
    if br.size == 0:
        br = np.zeros(2, np.uint32)
    rt = np.ascontiguousarray(read_type, dtype=np.uint8)
    view = _BadParts(len(names), name_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), blob,
                     lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                     bo.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                     br.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                     rt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return view, (blob, name_off, lengths, bo, br, rt)


def edit_file_to(op, in_path, sink, names, lengths, bad_offsets, bad_regions, read_type, n_threads=0):
    """yacrd_edit_file_to: the edited, uncompressed bytes go to `sink` instead of a file.  `sink` is a Python callable
    taking bytes (a false / None result = go on, anything true = stop: the edit fails) or a yacrd_byte_sink structure
    (GzipWriter.sink())."""
    lib = load_library()
    view, keep = _bad_parts(names, lengths, bad_offsets, bad_regions, read_type)
    if callable(sink):
        raised = []

        def _write(_ctx, p, n):
            try:
                return 1 if sink(ctypes.string_at(p, n)) else 0
            except Exception as exc:  # (an exception cannot cross the C frames: the edit stops, it is raised below)
                raised.append(exc)
                return 1
        cb = ByteSink.WRITE(_write)
        s = ByteSink(None, cb)
    else:
        raised = []
        s = sink
    rc = lib.yacrd_edit_file_to(op, in_path.encode(), ctypes.byref(view), n_threads, ctypes.addressof(s))
    del keep
    if raised:
        raise raised[0]
    _check(lib, rc)


def file_compression(path):
    """yacrd_file_compression: 0 none, 1 gzip, 2 bzip2, 3 xz, by the magic bytes."""
    return int(load_library().yacrd_file_compression(os.fsencode(path)))


def bgzf_encode_host(data):
    """yacrd_bgzf_encode_host: the device encoder's text run by one host thread; the bytes Engine.gzip gives."""
    lib = load_library()
    data = bytes(data)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    _check(lib, lib.yacrd_bgzf_encode_host(data, len(data), ctypes.byref(out), ctypes.byref(n)))
    try:
        return ctypes.string_at(out.value, int(n.value))
    finally:
        lib.yacrd_bytes_free(out)


def bgzf_decode_host(data):
    """yacrd_bgzf_decode_host: the device decoder's text run by one host thread; the bytes Engine.gunzip gives.  Raises
    HostError (the message names the cause) for a stream that is not BGZF or holds a member the decoder does not take."""
    lib = load_library()
    data = bytes(data)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    _check(lib, lib.yacrd_bgzf_decode_host(data, len(data), ctypes.byref(out), ctypes.byref(n)))
    try:
        return ctypes.string_at(out.value, int(n.value))
    finally:
        lib.yacrd_bytes_free(out)


GZIP_STREAM_COUNTERS = ("n_chunks", "n_spans", "n_false_starts", "rounds", "n_blocks", "out_bytes")


def gzip_stream_decode_host(data, chunk=0):
    """yacrd_gzip_stream_decode_host: the plain-gzip device decoder's text run by one host thread, block starts looked for
    per `chunk` compressed bytes (0: the default) -> (the text, {counter: value} with GZIP_STREAM_COUNTERS' names): the bytes
    and counters Engine.gunzip_stream gives.  Raises HostError (the message names the cause) for what is not one gzip member
    or a payload the decoder does not take."""
    lib = load_library()
    data = bytes(data)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    counters = (ctypes.c_uint64 * 6)()
    _check(lib, lib.yacrd_gzip_stream_decode_host(data, len(data), int(chunk), ctypes.byref(out), ctypes.byref(n), counters))
    try:
        return ctypes.string_at(out.value, int(n.value)), dict(zip(GZIP_STREAM_COUNTERS, (int(v) for v in counters)))
    finally:
        lib.yacrd_bytes_free(out)


def bgzf_plan_segments(data, landed, chunk=0, seg_chunks=0):
    """yacrd_bgzf_plan_segments: the segment-wise inflate's planner over a BGZF stream and a schedule of landed compressed
    bytes -> (members u64[M,4]: in_off, csize, isize, out_off; steps u64[S,8]: call, m0, m1, inflated, t0, t1, avail, last).
    chunk / seg_chunks 0: the mover's 4 MiB and 32."""
    lib = load_library()
    data = bytes(data)
    sched = np.ascontiguousarray(landed, dtype=np.uint64)
    mo, so = ctypes.c_void_p(), ctypes.c_void_p()
    nm, ns = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib, lib.yacrd_bgzf_plan_segments(data, len(data), sched.ctypes.data, len(sched), int(chunk), int(seg_chunks), ctypes.byref(mo),
                                             ctypes.byref(nm), ctypes.byref(so), ctypes.byref(ns)))
    try:
        members = np.frombuffer(ctypes.string_at(mo.value, int(nm.value) * 32), dtype=np.uint64).reshape(-1, 4).copy()
        steps = np.frombuffer(ctypes.string_at(so.value, int(ns.value) * 64), dtype=np.uint64).reshape(-1, 8).copy()
    finally:
        lib.yacrd_bytes_free(mo)
        lib.yacrd_bytes_free(so)
    return members, steps


def bgzf_text_ends(blob, delim):
    """yacrd_bgzf_text_ends: what the device overlap editor asks of a BGZF text before its first launch -> (the field count
    under `delim` (one byte, or its code) of the first non-empty line, 0 when there is none; whether the text's last byte is a
    newline, True for a text of no bytes).  Raises HostError for a stream that is not BGZF, a sampled member the decoder does
    not take, or a first non-empty line that is not complete within the first MiB of a text that goes on."""
    lib = load_library()
    blob = bytes(blob)
    d = delim if isinstance(delim, int) else ord(delim)
    nf, nl = ctypes.c_uint32(), ctypes.c_int()
    _check(lib, lib.yacrd_bgzf_text_ends(blob, len(blob), int(d), ctypes.byref(nf), ctypes.byref(nl)))
    return int(nf.value), bool(nl.value)


def bgzf_window_cuts(blob, W):
    """yacrd_bgzf_window_cuts: where the windows of a BGZF text end (csrc/bgzf_windows.h) -> [(m0, m1, c0, c1, t0, t1)], one
    per window: its members, its bytes of the compressed stream, its bytes of the text.  A window takes members while both
    its text and its stream bytes are at most W, and always one.  Raises HostError for a stream that is not BGZF and for
    W < 65 536."""
    lib = load_library()
    blob = bytes(blob)
    co, nc = ctypes.c_void_p(), ctypes.c_uint64()
    _check(lib, lib.yacrd_bgzf_window_cuts(blob, len(blob), int(W), ctypes.byref(co), ctypes.byref(nc)))
    try:
        cuts = np.frombuffer(ctypes.string_at(co.value, int(nc.value) * 48), dtype=np.uint64).reshape(-1, 6)
        return [tuple(int(x) for x in row) for row in cuts]
    finally:
        lib.yacrd_bytes_free(co)


EDIT_WHOLE, EDIT_WINDOWS, EDIT_FALLBACK = 0, 1, 2


def edit_window_route(n, window_switch, whole_fits, ring_fits):
    """yacrd_edit_window_route (csrc/edit_route.h): how the device overlap editor runs a plain text of `n` bytes
    -> (EDIT_WHOLE / EDIT_WINDOWS / EDIT_FALLBACK, the window's bytes, the mover's chunk: how far a line may reach into
    the next window).  window_switch: what Engine.debug_edit_window holds; whole_fits / ring_fits: whether the whole-text
    run and the ring of a run in windows find room.  Asks nothing of any device."""
    lib = load_library()
    W, C = ctypes.c_uint64(), ctypes.c_uint64()
    r = lib.yacrd_edit_window_route(int(n), int(window_switch), int(bool(whole_fits)), int(bool(ring_fits)), ctypes.byref(W), ctypes.byref(C))
    return int(r), int(W.value), int(C.value)


def deflate_code_lengths(freq, limit):
    """yacrd_deflate_code_lengths: the encoder's length-limited code lengths for a histogram."""
    lib = load_library()
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.zeros(len(f), np.uint8)
    _check(lib, lib.yacrd_deflate_code_lengths(f.ctypes.data, len(f), int(limit), out.ctypes.data))
    return out


def edit_file(op, in_path, out_path, names, lengths, bad_offsets, bad_regions, read_type, n_threads=0):
    """editor::{scrubbing,filter,extract,split} over the BadPart table (names, lengths, region CSR,
    engine read types).  n_threads: 0 = every usable CPU (plain FASTA / FASTQ are edited chunk-parallel)."""
    lib = load_library()
    blob = b"".join(n.encode() for n in names)
    name_off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(n.encode()) for n in names], out=name_off[1:])
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    bo = np.ascontiguousarray(bad_offsets, dtype=np.uint64)
    br = np.ascontiguousarray(bad_regions, dtype=np.uint32).reshape(-1)
    if br.size == 0:
        br = np.zeros(2, np.uint32)
    rt = np.ascontiguousarray(read_type, dtype=np.uint8)
    view = _BadParts(len(names), name_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), blob,
                     lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                     bo.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                     br.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                     rt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    _check(lib, lib.yacrd_edit_file_mt(op, in_path.encode(), out_path.encode(), ctypes.byref(view), n_threads))


def report_read(path):
    """FromReport: .yacrd -> (names, lengths u32, bad_offsets u64, bad_regions u32[G,2])."""
    lib = load_library()
    h = ctypes.c_void_p()
    _check(lib, lib.yacrd_report_read(path.encode(), ctypes.byref(h)))
    try:
        v = _BadParts()
        _check(lib, lib.yacrd_report_get(h, ctypes.byref(v)))
        R = int(v.n_reads)
        name_off = np.ctypeslib.as_array(v.name_off, shape=(R + 1,)).copy()
        blob = ctypes.string_at(v.names, int(name_off[-1])) if R else b""
        names = [blob[int(name_off[i]):int(name_off[i + 1])].decode() for i in range(R)]
        lengths = np.ctypeslib.as_array(v.lengths, shape=(R,)).copy() if R else np.zeros(0, np.uint32)
        bo = np.ctypeslib.as_array(v.bad_offsets, shape=(R + 1,)).copy()
        G = int(bo[-1])
        br = (np.ctypeslib.as_array(v.bad_regions, shape=(2 * G,)).copy().reshape(-1, 2)
              if G else np.zeros((0, 2), np.uint32))
    finally:
        lib.yacrd_report_free(h)
    return names, lengths, bo, br
