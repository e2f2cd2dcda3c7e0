"""ctypes binding of include/yacrd_engine.h (libyacrd_hip.so).  No CPU fallback."""
import ctypes
import os
import subprocess
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "lib", "libyacrd_hip.so")

NOT_BAD, CHIMERIC, NOT_COVERED = 0, 1, 2
TYPE_NAMES = {NOT_BAD: "NotBad", CHIMERIC: "Chimeric", NOT_COVERED: "NotCovered"}
# yacrd_engine_cfg.flags: the timing flags are part of include/yacrd_engine.h, everything else is an A/B or
# test switch from include/yacrd_engine_debug.h
F_FORCE_GENERAL = 1
F_FORCE_LDS_SORT = 2
F_WAVE_ONLY = 8
F_NO_HALVES = 16
F_TIMING_FULL = 32
F_NO_PREDICTION = 64
F_NO_PREFILTER = 256
F_COUNT_PREFILTERED = 512
F_NO_TIMING = 1024
F_BLOCKING_WAIT = 2048
F_NO_DEFER = 4096
F_ALWAYS_DEFER = 8192
F_TIMING_SAMPLED = 32768
F_STREAM_SCREEN = 65536
F_SCREEN_ITEMS_1 = 262144
F_SCREEN_ITEMS_2 = 524288
F_NO_FUSED_SCREEN = 1048576
F_SCREEN_WIDE = 2097152
F_SCREEN_DIRECT = 8388608  # the long launch takes H16 reads by index, the plan runs beside it: wherever legal (tests) ...
F_NO_SCREEN_DIRECT = 16777216  # ... never (A/B)
# debug symbols beside the flags (include/yacrd_engine_debug.h); EXPORTED_SYMBOLS below is yacrd_engine.h's list alone
DEBUG_SYMBOLS = [
    "yacrd_debug_sort_pairs", "yacrd_debug_last_counters", "yacrd_debug_last_input_csr", "yacrd_debug_peer_copy_counts",
    "yacrd_debug_live_bytes", "yacrd_debug_direct_runs", "yacrd_debug_big_routes",
    "yacrd_debug_seq_window", "yacrd_debug_seq_windows", "yacrd_debug_long_min_reads", "yacrd_debug_compute_units",
    "yacrd_debug_edit_window", "yacrd_debug_edit_windows", "yacrd_debug_gunzip_chunk",
]
F_ONE_LAUNCH = 4194304  # include/yacrd_engine.h: a short batch as ONE kernel launch (csrc/one_batch.h)

# every symbol include/yacrd_engine.h declares
EXPORTED_SYMBOLS = [
    "yacrd_abi_version", "yacrd_last_error", "yacrd_engine_create", "yacrd_engine_destroy",
    "yacrd_engine_run", "yacrd_result_free", "yacrd_engine_run_device", "yacrd_engine_fetch",
    "yacrd_engine_last_timing", "yacrd_partition_reads", "yacrd_engine_classify",
    "yacrd_engines_run_partitioned", "yacrd_engine_timing_total", "yacrd_engine_event_overhead", "yacrd_engine_submit_device", "yacrd_engine_wait", "yacrd_engines_run_device_batches",
    "yacrd_engine_submit", "yacrd_engine_collect", "yacrd_pinned_alloc", "yacrd_pinned_free",
    "yacrd_stream_open", "yacrd_stream_sink", "yacrd_stream_acquire", "yacrd_stream_commit",
    "yacrd_stream_finish", "yacrd_stream_last_stats", "yacrd_stream_reset", "yacrd_stream_close",
    "yacrd_engine_ingest_paf", "yacrd_engine_ingest_overlaps", "yacrd_engine_ingest_overlaps_mem", "yacrd_engines_ingest_overlaps",
    "yacrd_engines_ingest_overlaps_mem", "yacrd_reads_free", "yacrd_engine_trim",
    "yacrd_engine_ingest_overlaps_bgzf_mem", "yacrd_engine_ingest_report_bgzf_mem",
    "yacrd_engine_ingest_report", "yacrd_engine_ingest_report_mem", "yacrd_engine_write_report", "yacrd_engine_write_report_mem",
    "yacrd_engine_edit_overlaps", "yacrd_engine_edit_overlaps_mem", "yacrd_edit_text_free",
    "yacrd_engine_edit_overlaps_gzip_mem", "yacrd_engine_edit_overlaps_gzip_file",
    "yacrd_engine_edit_overlaps_bgzf_mem", "yacrd_engine_edit_overlaps_bgzf_file",
    "yacrd_engine_edit_overlaps_resident_mem", "yacrd_engine_edit_overlaps_resident_file",
    "yacrd_engine_edit_fastq", "yacrd_engine_edit_fastq_mem", "yacrd_engine_edit_fastq_gzip_mem", "yacrd_engine_edit_fastq_gzip_file",
    "yacrd_engine_edit_fasta", "yacrd_engine_edit_fasta_mem", "yacrd_engine_edit_fasta_gzip_mem", "yacrd_engine_edit_fasta_gzip_file",
    "yacrd_engine_gunzip_mem", "yacrd_engine_edit_fastq_bgzf_mem", "yacrd_engine_edit_fastq_bgzf_file",
    "yacrd_engine_edit_fasta_bgzf_mem", "yacrd_engine_edit_fasta_bgzf_file", "yacrd_engine_gunzip_stream_mem",
    "yacrd_engine_edit_fastq_gz_mem", "yacrd_engine_edit_fastq_gz_file", "yacrd_engine_edit_fasta_gz_mem", "yacrd_engine_edit_fasta_gz_file",
    "yacrd_engine_gzip_mem", "yacrd_gzip_writer_open", "yacrd_gzip_writer_write", "yacrd_gzip_writer_sink", "yacrd_gzip_writer_close",
    "yacrd_gzip_writer_abort",
    "yacrd_stream_device_of", "yacrd_stream_group_open", "yacrd_stream_group_sink", "yacrd_stream_group_finish",
    "yacrd_stream_group_last_stats", "yacrd_stream_group_reset", "yacrd_stream_group_close",
]


class EngineError(RuntimeError):
    pass


class NeedsHostParser(EngineError):
    """yacrd_engine_ingest_paf returned YACRD_EFALLBACK: the input is for the host parser."""


E_FALLBACK = 5


class _Reads(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_uint64), ("n_records", ctypes.c_uint64),
                ("lengths", ctypes.POINTER(ctypes.c_uint32)), ("name_off", ctypes.POINTER(ctypes.c_uint64)),
                ("names", ctypes.POINTER(ctypes.c_char))]


class _ReportTable(ctypes.Structure):  # yacrd_report_table
    _fields_ = [("n_reads", ctypes.c_uint64)] + \
               [(n, ctypes.c_void_p) for n in ("name_off", "names", "lengths", "bad_offsets", "bad_regions", "read_type")]


class _ReportWriteStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_reads", "n_regions", "text_bytes")] + \
               [(n, ctypes.c_float) for n in ("up_ms", "kernel_ms", "out_ms")] + [("resident", ctypes.c_uint32)]


class _IngestStats(ctypes.Structure):
    _fields_ = [("text_bytes", ctypes.c_uint64), ("n_records", ctypes.c_uint64), ("n_reads", ctypes.c_uint64)] + \
               [(n, ctypes.c_float) for n in ("text_ms", "parse_ms", "build_ms", "run_ms", "d2h_ms")]


class _TypeTable(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_uint64), ("name_off", ctypes.c_void_p), ("names", ctypes.c_void_p), ("read_type", ctypes.c_void_p)]


class _EditStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("text_bytes", "kept_bytes", "n_lines", "n_kept")] + \
               [(n, ctypes.c_float) for n in ("text_ms", "table_ms", "kernel_ms", "out_ms")] + [("mirror_reused", ctypes.c_uint32)]


class _SeqEditStats(ctypes.Structure):  # yacrd_seq_edit_stats
    _fields_ = [(n, ctypes.c_uint64) for n in ("text_bytes", "out_bytes", "n_records", "n_out_records")] + \
               [(n, ctypes.c_float) for n in ("text_ms", "table_ms", "kernel_ms", "out_ms")]


class _GzipStats(ctypes.Structure):
    _fields_ = [("in_bytes", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64), ("n_members", ctypes.c_uint64), ("n_stored", ctypes.c_uint64),
                ("h2d_ms", ctypes.c_float), ("kernel_ms", ctypes.c_float), ("d2h_ms", ctypes.c_float), ("write_ms", ctypes.c_float)]


class _GunzipStats(ctypes.Structure):  # yacrd_gunzip_stats
    _fields_ = [(n, ctypes.c_uint64) for n in ("in_bytes", "out_bytes", "n_members")] + \
               [(n, ctypes.c_float) for n in ("walk_ms", "h2d_ms", "kernel_ms", "d2h_ms")]


class _GunzipStreamStats(ctypes.Structure):  # yacrd_gunzip_stream_stats
    _fields_ = [(n, ctypes.c_uint64) for n in ("in_bytes", "out_bytes", "n_chunks", "n_spans", "n_false_starts", "rounds", "n_blocks")] + \
               [(n, ctypes.c_float) for n in ("find_ms", "size_ms", "symbols_ms", "windows_ms", "bytes_ms", "h2d_ms", "d2h_ms")]


from .host import ByteSink  # noqa: E402  (yacrd_byte_sink: one structure, declared in both headers)


class _Cfg(ctypes.Structure):
    _fields_ = [("device_id", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class _Result(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_uint64), ("n_regions", ctypes.c_uint64),
                ("bad_offsets", ctypes.POINTER(ctypes.c_uint64)),
                ("bad_regions", ctypes.POINTER(ctypes.c_uint32)),
                ("read_type", ctypes.POINTER(ctypes.c_uint8))]


class _DevResult(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_uint64), ("n_regions", ctypes.c_uint64),
                ("d_bad_offsets", ctypes.c_void_p), ("d_bad_regions", ctypes.c_void_p),
                ("d_read_type", ctypes.c_void_p)]


class DeviceBatch(ctypes.Structure):
    """yacrd_device_batch: a CSR resident in HBM + the run's parameters."""
    _fields_ = [("d_offsets", ctypes.c_void_p), ("d_intervals", ctypes.c_void_p), ("d_lengths", ctypes.c_void_p),
                ("n_reads", ctypes.c_uint64), ("n_intervals", ctypes.c_uint64), ("coverage", ctypes.c_uint32),
                ("not_coverage", ctypes.c_double)]


BATCH_DONE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                              ctypes.POINTER(_DevResult))


class _Timing(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in
                ("h2d_ms", "plan_ms", "sweep_small_ms", "sweep_medium_ms", "sweep_general_ms",
                 "compact_ms", "d2h_ms", "total_ms")] + \
               [(n, ctypes.c_uint64) for n in
                ("n_small", "n_medium", "n_general", "iv_small", "iv_medium", "iv_general")] + \
               [("class_ms", ctypes.c_float * 12), ("class_reads", ctypes.c_uint64 * 12),
                ("class_intervals", ctypes.c_uint64 * 12), ("fused_ms", ctypes.c_float),
                ("fused_reads", ctypes.c_uint64), ("fused_intervals", ctypes.c_uint64),
                ("prefiltered_reads", ctypes.c_uint64), ("deferred_reads", ctypes.c_uint64),
                ("deferred_intervals", ctypes.c_uint64), ("screened", ctypes.c_uint32),
                ("timed_runs", ctypes.c_uint32), ("screen_items", ctypes.c_uint32), ("screen_wide", ctypes.c_uint32),
                ("one_launch", ctypes.c_uint32), ("fused_reruns", ctypes.c_uint32),
                ("predicted", ctypes.c_uint32), ("prediction_misses", ctypes.c_uint32),
                ("build_switches", ctypes.c_uint32), ("sorting_build", ctypes.c_uint32)]

CLASS_NAMES = "R2,R4,R8,R16,H16,W2,W4,W8,W16,M1,M2,BIG".split(",")
CLASS_KERNELS = {  # the HIP kernel behind each class, as rocprofv3 prints it
    # (R2..H16 share one launch: yacrd_timing.fused_ms; its screening builds are named in bench.py)
    "R2": "sweep_small_fused_kernel", "R4": "sweep_small_fused_kernel", "R8": "sweep_small_fused_kernel",
    "R16": "sweep_small_fused_kernel", "H16": "sweep_small_fused_kernel",
    "W2": "sweep_group_kernel<64, 2>", "W4": "sweep_group_kernel<64, 4>", "W8": "sweep_group_kernel<64, 8>",
    "W16": "sweep_group_kernel<64, 16>",
    # the workgroup classes: the screen, then the fallback of what it leaves (two launches since round 6: screen_wg.h); the bracket
    # also holds the (usually empty) sweep_lds_kernel<1024, 32768> behind it for M2
    "M1": "screen_wg_kernel + screen_wg_fused_kernel over what it leaves",
    "M2": "screen_wg_kernel + screen_wg_fused_kernel over what it leaves (+ sweep_lds_kernel<1024, 32768> over what exceeds 16 384 events)",
    "BIG": "bs_setup / bs_minmax / bs_hist / bs_verdict (screen_big.h)",
}


class _StreamStats(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64), ("h2d_bytes", ctypes.c_uint64),
                ("h2d_busy_ms", ctypes.c_float), ("build_ms", ctypes.c_float),
                ("run_ms", ctypes.c_float), ("d2h_ms", ctypes.c_float)]


class OvlRec(ctypes.Structure):
    """yacrd_ovl_rec: one overlap line, both reads (handles) and their intervals."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("a", "b", "sa", "ea", "sb", "eb")]


_ACQUIRE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(OvlRec)),
                            ctypes.POINTER(ctypes.c_uint64))
_COMMIT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(OvlRec), ctypes.c_uint64)


class RecSink(ctypes.Structure):
    """yacrd_rec_sink"""
    _fields_ = [("ctx", ctypes.c_void_p), ("acquire", _ACQUIRE), ("commit", _COMMIT)]


OVL_REC_DTYPE = np.dtype([(n, np.uint32) for n in ("a", "b", "sa", "ea", "sb", "eb")])

Result = namedtuple("Result", "bad_offsets bad_regions read_type")

_lib = None


def lib_path():
    return _LIB


def build(force=False):
    """Compile libyacrd_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-s", "-C", os.path.join(_HERE, "csrc")]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return _LIB


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so.7 (+ HSA runtime).  Two HIP runtimes in one
    process cannot both own the GPU ("No HIP GPUs are available" for whichever comes second), so
    when torch is installed we load ITS copy first (RTLD_GLOBAL); our DT_NEEDED libamdhip64.so.7
    then binds to that already-loaded SONAME.  Without torch (e.g. the C++ CLI) the library uses
    /opt/rocm's runtime through its RUNPATH.  Set YACRD_HIP_RUNTIME=system to skip this."""
    if os.environ.get("YACRD_HIP_RUNTIME", "") == "system":
        return None
    import importlib.util
    import sys
    try:
        if "torch" in sys.modules:
            tdir = os.path.dirname(sys.modules["torch"].__file__)
        else:
            spec = importlib.util.find_spec("torch")
            if spec is None or not spec.origin:
                return None
            tdir = os.path.dirname(spec.origin)
    except (ImportError, ValueError):
        return None
    cand = os.path.join(tdir, "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return None
    try:
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except OSError:
        return None
    return cand


def peer_copy_counts():
    """yacrd_debug_peer_copy_counts (tests): cross-engine copies of the N-engine device parser by route:
    [same device, hipMemcpyPeerAsync, staged through the host]."""
    lib = load_library()
    out = (ctypes.c_uint64 * 3)()
    lib.yacrd_debug_peer_copy_counts.restype = None
    lib.yacrd_debug_peer_copy_counts(out)
    return [int(x) for x in out]


def live_bytes():
    """yacrd_debug_live_bytes (tests): bytes the library holds right now, process-wide: (device memory, pinned host memory)."""
    lib = load_library()
    out = (ctypes.c_uint64 * 2)()
    lib.yacrd_debug_live_bytes.restype = None
    lib.yacrd_debug_live_bytes(out)
    return (int(out[0]), int(out[1]))


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise EngineError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % _LIB)
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_LIB)
    u64p, u32p, u8p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint8))
    lib.yacrd_abi_version.restype = ctypes.c_int
    lib.yacrd_last_error.restype = ctypes.c_char_p
    lib.yacrd_engine_create.argtypes = [ctypes.POINTER(_Cfg), ctypes.POINTER(ctypes.c_void_p)]
    lib.yacrd_engine_destroy.argtypes = [ctypes.c_void_p]
    lib.yacrd_engine_destroy.restype = None
    lib.yacrd_engine_run.argtypes = [ctypes.c_void_p, u64p, u32p, u32p, ctypes.c_uint64,
                                     ctypes.c_uint32, ctypes.c_double, ctypes.POINTER(_Result)]
    lib.yacrd_result_free.argtypes = [ctypes.POINTER(_Result)]
    lib.yacrd_result_free.restype = None
    lib.yacrd_engine_run_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                            ctypes.c_uint32, ctypes.c_double,
                                            ctypes.POINTER(_DevResult)]
    lib.yacrd_engine_submit_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.c_uint32, ctypes.c_double]
    lib.yacrd_engine_wait.argtypes = [ctypes.c_void_p, ctypes.POINTER(_DevResult)]
    lib.yacrd_engines_run_device_batches.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
                                                     ctypes.POINTER(DeviceBatch), ctypes.c_uint32, BATCH_DONE,
                                                     ctypes.c_void_p, ctypes.POINTER(_DevResult)]
    lib.yacrd_engine_fetch.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Result)]
    lib.yacrd_engine_ingest_paf.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_double,
                                            ctypes.POINTER(_Result), ctypes.POINTER(_Reads), ctypes.POINTER(_IngestStats)]
    lib.yacrd_engine_ingest_overlaps.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                                                 ctypes.c_double, ctypes.POINTER(_Result), ctypes.POINTER(_Reads),
                                                 ctypes.POINTER(_IngestStats)]
    lib.yacrd_engine_ingest_overlaps_mem.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_uint32, ctypes.c_double, ctypes.POINTER(_Result), ctypes.POINTER(_Reads),
                                                     ctypes.POINTER(_IngestStats)]
    lib.yacrd_engines_ingest_overlaps.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_uint32, ctypes.c_double, ctypes.POINTER(_Result),
                                                  ctypes.POINTER(_Reads), ctypes.POINTER(_IngestStats)]
    lib.yacrd_engines_ingest_overlaps_mem.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                                      ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_double,
                                                      ctypes.POINTER(_Result), ctypes.POINTER(_Reads), ctypes.POINTER(_IngestStats)]
    lib.yacrd_engine_ingest_report.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_double, ctypes.POINTER(_Result),
                                               ctypes.POINTER(_Reads), ctypes.POINTER(_IngestStats)]
    lib.yacrd_engine_ingest_report_mem.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_double,
                                                   ctypes.POINTER(_Result), ctypes.POINTER(_Reads), ctypes.POINTER(_IngestStats)]
    lib.yacrd_engine_ingest_overlaps_bgzf_mem.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_uint32, ctypes.c_double, ctypes.POINTER(_Result), ctypes.POINTER(_Reads),
                                                          ctypes.POINTER(_IngestStats), ctypes.POINTER(_GunzipStats)]
    lib.yacrd_engine_ingest_report_bgzf_mem.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_double,
                                                        ctypes.POINTER(_Result), ctypes.POINTER(_Reads), ctypes.POINTER(_IngestStats),
                                                        ctypes.POINTER(_GunzipStats)]
    lib.yacrd_engine_write_report.argtypes = [ctypes.c_void_p, ctypes.POINTER(_ReportTable), ctypes.c_char_p,
                                              ctypes.POINTER(_ReportWriteStats)]
    lib.yacrd_engine_write_report_mem.argtypes = [ctypes.c_void_p, ctypes.POINTER(_ReportTable), ctypes.POINTER(ctypes.c_void_p),
                                                  ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_ReportWriteStats)]
    lib.yacrd_debug_sort_pairs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    lib.yacrd_engine_trim.argtypes = [ctypes.c_void_p]
    lib.yacrd_engine_edit_overlaps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(_TypeTable), ctypes.POINTER(_EditStats)]
    lib.yacrd_engine_edit_overlaps_mem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                   ctypes.POINTER(_TypeTable), ctypes.POINTER(ctypes.c_void_p),
                                                   ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_EditStats)]
    lib.yacrd_engine_edit_overlaps_gzip_mem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                        ctypes.POINTER(_TypeTable), ctypes.POINTER(ctypes.c_void_p),
                                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_EditStats), ctypes.POINTER(_GzipStats)]
    lib.yacrd_engine_edit_overlaps_gzip_file.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                         ctypes.POINTER(_TypeTable), ctypes.c_char_p, ctypes.POINTER(_EditStats),
                                                         ctypes.POINTER(_GzipStats)]
    lib.yacrd_engine_edit_overlaps_bgzf_mem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                        ctypes.POINTER(_TypeTable), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_EditStats), ctypes.POINTER(_GzipStats),
                                                        ctypes.POINTER(_GunzipStats)]
    lib.yacrd_engine_edit_overlaps_bgzf_file.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                         ctypes.POINTER(_TypeTable), ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(_EditStats),
                                                         ctypes.POINTER(_GzipStats), ctypes.POINTER(_GunzipStats)]
    lib.yacrd_engine_edit_overlaps_resident_mem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_TypeTable), ctypes.c_int,
                                                            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                                            ctypes.POINTER(_EditStats), ctypes.POINTER(_GzipStats)]
    lib.yacrd_engine_edit_overlaps_resident_file.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_TypeTable), ctypes.c_int,
                                                             ctypes.c_char_p, ctypes.POINTER(_EditStats), ctypes.POINTER(_GzipStats)]
    lib.yacrd_edit_text_free.argtypes = [ctypes.c_void_p]
    lib.yacrd_engine_edit_fastq.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                            ctypes.POINTER(_ReportTable), ctypes.POINTER(_SeqEditStats)]
    lib.yacrd_engine_edit_fastq_mem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(_ReportTable),
                                                ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                                ctypes.POINTER(_SeqEditStats)]
    lib.yacrd_engine_edit_fastq_gzip_mem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                                     ctypes.POINTER(_ReportTable), ctypes.POINTER(ctypes.c_void_p),
                                                     ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_SeqEditStats),
                                                     ctypes.POINTER(_GzipStats)]
    lib.yacrd_engine_edit_fastq_gzip_file.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                                      ctypes.POINTER(_ReportTable), ctypes.c_char_p, ctypes.POINTER(_SeqEditStats),
                                                      ctypes.POINTER(_GzipStats)]
    for fq, fa in ((getattr(lib, "yacrd_engine_edit_fastq" + form), getattr(lib, "yacrd_engine_edit_fasta" + form))
                   for form in ("", "_mem", "_gzip_mem", "_gzip_file")):
        fa.argtypes = fq.argtypes  # (the FASTA calls take what the FASTQ calls take)
    lib.yacrd_edit_text_free.restype = None
    lib.yacrd_engine_gunzip_mem.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_GunzipStats)]
    lib.yacrd_engine_gunzip_stream_mem.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p),
                                                   ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_GunzipStreamStats)]
    for fmt in ("fastq", "fasta"):  # (the gzip forms' arguments and a trailing yacrd_gunzip_stats)
        for form in ("mem", "file"):
            getattr(lib, "yacrd_engine_edit_%s_bgzf_%s" % (fmt, form)).argtypes = \
                getattr(lib, "yacrd_engine_edit_%s_gzip_%s" % (fmt, form)).argtypes + [ctypes.POINTER(_GunzipStats)]
            getattr(lib, "yacrd_engine_edit_%s_gz_%s" % (fmt, form)).argtypes = \
                getattr(lib, "yacrd_engine_edit_%s_gzip_%s" % (fmt, form)).argtypes + [ctypes.POINTER(_GunzipStreamStats)]
    lib.yacrd_engine_gzip_mem.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_GzipStats)]
    lib.yacrd_gzip_writer_open.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
    lib.yacrd_gzip_writer_write.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    lib.yacrd_gzip_writer_sink.argtypes = [ctypes.c_void_p, ctypes.POINTER(ByteSink)]
    lib.yacrd_gzip_writer_close.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GzipStats)]
    lib.yacrd_gzip_writer_abort.argtypes = [ctypes.c_void_p]
    lib.yacrd_gzip_writer_abort.restype = None
    lib.yacrd_reads_free.argtypes = [ctypes.POINTER(_Reads)]
    lib.yacrd_reads_free.restype = None
    lib.yacrd_stream_reset.argtypes = [ctypes.c_void_p]
    lib.yacrd_engine_last_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Timing)]
    lib.yacrd_partition_reads.argtypes = [u64p, ctypes.c_uint64, ctypes.c_uint32, u64p]
    lib.yacrd_engine_classify.argtypes = [ctypes.c_void_p, u64p, u32p, u32p, ctypes.c_uint64,
                                          ctypes.c_double, u8p]
    lib.yacrd_engine_event_overhead.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.yacrd_engine_event_overhead.restype = ctypes.c_int
    lib.yacrd_engine_timing_total.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Timing),
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    lib.yacrd_engines_run_partitioned.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
                                                  u64p, u32p, u32p, ctypes.c_uint64,
                                                  ctypes.c_uint32, ctypes.c_double,
                                                  ctypes.POINTER(_Result)]
    lib.yacrd_engine_submit.argtypes = [ctypes.c_void_p, u64p, u32p, u32p, ctypes.c_uint64,
                                        ctypes.c_uint32, ctypes.c_double]
    lib.yacrd_engine_collect.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Result)]
    lib.yacrd_pinned_alloc.argtypes = [ctypes.c_size_t]
    lib.yacrd_pinned_alloc.restype = ctypes.c_void_p
    lib.yacrd_pinned_free.argtypes = [ctypes.c_void_p]
    lib.yacrd_pinned_free.restype = None
    lib.yacrd_stream_open.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.POINTER(ctypes.c_void_p)]
    lib.yacrd_stream_sink.argtypes = [ctypes.c_void_p, ctypes.POINTER(RecSink)]
    lib.yacrd_stream_acquire.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(OvlRec)),
                                         ctypes.POINTER(ctypes.c_uint64)]
    lib.yacrd_stream_commit.argtypes = [ctypes.c_void_p, ctypes.POINTER(OvlRec), ctypes.c_uint64]
    lib.yacrd_stream_finish.argtypes = [ctypes.c_void_p, u32p, ctypes.c_uint64, u32p, ctypes.c_uint64,
                                        ctypes.c_uint32, ctypes.c_double, ctypes.POINTER(_Result)]
    lib.yacrd_stream_last_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(_StreamStats)]
    lib.yacrd_stream_close.argtypes = [ctypes.c_void_p]
    lib.yacrd_stream_close.restype = None
    lib.yacrd_stream_device_of.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.yacrd_stream_device_of.restype = ctypes.c_uint32
    lib.yacrd_stream_group_open.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_uint64,
                                            ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
    lib.yacrd_stream_group_sink.argtypes = [ctypes.c_void_p, ctypes.POINTER(RecSink)]
    lib.yacrd_stream_group_finish.argtypes = lib.yacrd_stream_finish.argtypes
    lib.yacrd_stream_group_last_stats.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(_StreamStats),
                                                  ctypes.POINTER(ctypes.c_uint64)]
    lib.yacrd_stream_group_reset.argtypes = [ctypes.c_void_p]
    lib.yacrd_stream_group_close.argtypes = [ctypes.c_void_p]
    lib.yacrd_stream_group_close.restype = None
    _lib = lib
    return lib


def _check(lib, rc):
    if rc != 0:
        raise EngineError("yacrd engine error %d: %s" % (rc, lib.yacrd_last_error().decode()))


def _ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _take(lib, res):
    R, G = int(res.n_reads), int(res.n_regions)
    bo = np.ctypeslib.as_array(res.bad_offsets, shape=(R + 1,)).copy()
    br = (np.ctypeslib.as_array(res.bad_regions, shape=(2 * G,)).copy().reshape(-1, 2)
          if G else np.zeros((0, 2), dtype=np.uint32))
    rt = np.ctypeslib.as_array(res.read_type, shape=(R,)).copy() if R else np.zeros(0, np.uint8)
    lib.yacrd_result_free(ctypes.byref(res))
    return Result(bo, br, rt)


def partition_reads(offsets, n_parts):
    """Contiguous read ranges balanced by interval count; no GPU needed."""
    lib = load_library()
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    cuts = np.zeros(n_parts + 1, dtype=np.uint64)
    _check(lib, lib.yacrd_partition_reads(_ptr(offsets, ctypes.c_uint64), offsets.shape[0] - 1,
                                          n_parts, _ptr(cuts, ctypes.c_uint64)))
    return cuts


def run_partitioned(engines, offsets, intervals, lengths, coverage, not_coverage):
    """Read-partitioned run over several engines (one per GPU); same output as one engine."""
    lib = load_library()
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    intervals = np.ascontiguousarray(intervals, dtype=np.uint32).reshape(-1)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    if intervals.size == 0:
        intervals = np.zeros(2, dtype=np.uint32)
    handles = (ctypes.c_void_p * len(engines))(*[e._h for e in engines])
    res = _Result()
    _check(lib, lib.yacrd_engines_run_partitioned(
        handles, len(engines), _ptr(offsets, ctypes.c_uint64), _ptr(intervals, ctypes.c_uint32),
        _ptr(lengths, ctypes.c_uint32), offsets.shape[0] - 1, min(int(coverage), 0xFFFFFFFF),
        float(not_coverage), ctypes.byref(res)))
    return _take(lib, res)


def ingest_overlaps(engines, source, coverage, not_coverage, n_threads=0, fmt=1):
    """yacrd_engines_ingest_overlaps[_mem]: overlap text -> (Result, names, lengths, stats), every engine parsing a byte
    range of the text and sweeping a range of the reads.  `source`: a path, bytes, or (address, n_bytes) of text in host
    memory.  Raises NeedsHostParser when the input is not for the device parser."""
    lib = load_library()
    handles = (ctypes.c_void_p * len(engines))(*[e._h for e in engines])
    res, rd, st = _Result(), _Reads(), _IngestStats()
    cov = min(int(coverage), 0xFFFFFFFF)
    if isinstance(source, (str, os.PathLike)):
        rc = lib.yacrd_engines_ingest_overlaps(handles, len(engines), os.fsencode(source), int(fmt), int(n_threads), cov,
                                               float(not_coverage), ctypes.byref(res), ctypes.byref(rd), ctypes.byref(st))
    else:
        if isinstance(source, tuple):
            addr, n, keep = int(source[0]), int(source[1]), None
        else:
            keep = ctypes.create_string_buffer(bytes(source), len(source))
            addr, n = ctypes.addressof(keep), len(source)
        rc = lib.yacrd_engines_ingest_overlaps_mem(handles, len(engines), addr, n, int(fmt), int(n_threads), cov, float(not_coverage),
                                                   ctypes.byref(res), ctypes.byref(rd), ctypes.byref(st))
        del keep
    return engines[0]._ingested(rc, res, rd, st)


def run_device_batches(engines, batches, done=None):
    """yacrd_engines_run_device_batches: `batches` = sequence of (d_offsets, d_intervals, d_lengths,
    n_reads, n_intervals, coverage, not_coverage) with device pointers; batch i runs on
    engines[i % len(engines)], len(engines) of them in flight; done(batch_index, engine) is called in
    order after each batch's wait (return True to stop).  Returns the last batch's device result."""
    lib = load_library()
    arr = (DeviceBatch * len(batches))()
    for i, b in enumerate(batches):
        arr[i] = DeviceBatch(b[0], b[1], b[2], b[3], b[4], min(int(b[5]), 0xFFFFFFFF), float(b[6]))
    handles = (ctypes.c_void_p * len(engines))(*[e._h for e in engines])
    by_handle = {e._h.value: e for e in engines}
    cb = BATCH_DONE(lambda user, i, h, res: 1 if done(i, by_handle[h]) else 0) if done else BATCH_DONE()
    out = _DevResult()
    _check(lib, lib.yacrd_engines_run_device_batches(handles, len(engines), arr, len(batches), cb, None,
                                                     ctypes.byref(out)))
    return out


class Engine:
    """One engine per GPU.  Mirrors the BadPart lifecycle: run() == compute_all_bad_part()."""

    def __init__(self, device_id=-1, flags=0):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        self.device_id = device_id
        cfg = _Cfg(device_id, flags)
        _check(self._lib, self._lib.yacrd_engine_create(ctypes.byref(cfg), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.yacrd_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, offsets, intervals, lengths, coverage, not_coverage):
        """Host CSR in, host CSR out (H2D + kernels + D2H)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        intervals = np.ascontiguousarray(intervals, dtype=np.uint32).reshape(-1)
        lengths = np.asarray(lengths)
        if lengths.size and int(lengths.max()) > 0xFFFFFFFF:
            raise EngineError("read length >= 2^32 is not supported by the engine ABI")
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        n_reads = offsets.shape[0] - 1
        if lengths.shape[0] != n_reads or intervals.shape[0] != 2 * int(offsets[-1]):
            raise EngineError("malformed CSR")
        res = _Result()
        _check(self._lib, self._lib.yacrd_engine_run(
            self._h, _ptr(offsets, ctypes.c_uint64), _ptr(intervals, ctypes.c_uint32),
            _ptr(lengths, ctypes.c_uint32), n_reads, min(int(coverage), 0xFFFFFFFF),
            float(not_coverage), ctypes.byref(res)))
        return _take(self._lib, res)

    def run_device(self, d_offsets, d_intervals, d_lengths, n_reads, n_intervals, coverage,
                   not_coverage):
        """Inputs are raw device pointers (ints).  Returns (n_regions, ptrs) without D2H."""
        out = _DevResult()
        _check(self._lib, self._lib.yacrd_engine_run_device(
            self._h, d_offsets, d_intervals, d_lengths, n_reads, n_intervals,
            min(int(coverage), 0xFFFFFFFF), float(not_coverage), ctypes.byref(out)))
        return out

    def submit_device(self, d_offsets, d_intervals, d_lengths, n_reads, n_intervals, coverage,
                      not_coverage):
        """run_device without the final wait (see yacrd_engine_submit_device); pair with wait()."""
        _check(self._lib, self._lib.yacrd_engine_submit_device(
            self._h, d_offsets, d_intervals, d_lengths, n_reads, n_intervals,
            min(int(coverage), 0xFFFFFFFF), float(not_coverage)))

    def wait(self):
        out = _DevResult()
        _check(self._lib, self._lib.yacrd_engine_wait(self._h, ctypes.byref(out)))
        return out

    def ingest_paf(self, path, coverage, not_coverage, n_threads=0, fmt=1):
        """yacrd_engine_ingest_overlaps (fmt 1 = PAF, 2 = M4, 0 = by file name): overlap text -> (Result, names,
        lengths, stats) with the parse on the GPU; raises NeedsHostParser when the input is not for the device parser."""
        res, rd, st = _Result(), _Reads(), _IngestStats()
        rc = self._lib.yacrd_engine_ingest_overlaps(self._h, os.fsencode(path), int(fmt), int(n_threads),
                                                    min(int(coverage), 0xFFFFFFFF), float(not_coverage), ctypes.byref(res),
                                                    ctypes.byref(rd), ctypes.byref(st))
        return self._ingested(rc, res, rd, st)

    def ingest_text(self, text, coverage, not_coverage, n_threads=0, fmt=1):
        """yacrd_engine_ingest_overlaps_mem: the same over text in host memory — `text`: bytes, or (address, n_bytes) of
        a buffer such as host.text_from_file's (a compressed overlap file, inflated)."""
        res, rd, st = _Result(), _Reads(), _IngestStats()
        if isinstance(text, tuple):
            addr, n = int(text[0]), int(text[1])
            keep = None
        else:
            keep = ctypes.create_string_buffer(bytes(text), len(text))
            addr, n = ctypes.addressof(keep), len(text)
        rc = self._lib.yacrd_engine_ingest_overlaps_mem(self._h, addr, n, int(fmt), int(n_threads), min(int(coverage), 0xFFFFFFFF),
                                                        float(not_coverage), ctypes.byref(res), ctypes.byref(rd), ctypes.byref(st))
        del keep
        return self._ingested(rc, res, rd, st)

    def ingest_report(self, path_or_bytes, not_coverage, n_threads=0):
        """yacrd_engine_ingest_report (a path: str / os.PathLike) or yacrd_engine_ingest_report_mem (bytes, or (address,
        n_bytes) of a buffer such as host.text_from_file's): a .yacrd report -> (Result, names, lengths, stats) as from
        ingest_paf / ingest_text, parsed, deduplicated and classified on the GPU (FromReport, src/stack.rs:176-257); raises
        NeedsHostParser when the report is for host.report_read + classify."""
        res, rd, st = _Result(), _Reads(), _IngestStats()
        if isinstance(path_or_bytes, (str, os.PathLike)):
            rc = self._lib.yacrd_engine_ingest_report(self._h, os.fsencode(path_or_bytes), int(n_threads), float(not_coverage),
                                                      ctypes.byref(res), ctypes.byref(rd), ctypes.byref(st))
            return self._ingested(rc, res, rd, st)
        if isinstance(path_or_bytes, tuple):
            addr, n = int(path_or_bytes[0]), int(path_or_bytes[1])
            keep = None
        else:
            keep = ctypes.create_string_buffer(bytes(path_or_bytes), len(path_or_bytes))
            addr, n = ctypes.addressof(keep), len(path_or_bytes)
        rc = self._lib.yacrd_engine_ingest_report_mem(self._h, addr, n, int(n_threads), float(not_coverage), ctypes.byref(res),
                                                      ctypes.byref(rd), ctypes.byref(st))
        del keep
        return self._ingested(rc, res, rd, st)

    def ingest_bgzf(self, blob, coverage, not_coverage, n_threads=0, fmt=1):
        """yacrd_engine_ingest_overlaps_bgzf_mem: ingest_text over a BGZF stream (bytes, or (address, n_bytes)) as it is — the
        compressed bytes go up and are inflated in HBM while they land.  (Result, names, lengths, stats) as from ingest_text
        of the inflated text; stats["inflate"]: the inflate's figures (n_members, in_bytes, out_bytes, walk_ms, h2d_ms,
        kernel_ms).  Raises NeedsHostParser, with nothing returned, when `blob` is not BGZF, holds a member the device decoder
        does not take, or inflates to a text ingest_text refuses."""
        res, rd, st, us = _Result(), _Reads(), _IngestStats(), _GunzipStats()
        addr, n, keep = self._host_bytes(blob)
        rc = self._lib.yacrd_engine_ingest_overlaps_bgzf_mem(self._h, addr, n, int(fmt), int(n_threads), min(int(coverage), 0xFFFFFFFF),
                                                             float(not_coverage), ctypes.byref(res), ctypes.byref(rd), ctypes.byref(st),
                                                             ctypes.byref(us))
        del keep
        return self._ingested(rc, res, rd, st, us)

    def ingest_report_bgzf(self, blob, not_coverage, n_threads=0):
        """yacrd_engine_ingest_report_bgzf_mem: ingest_report over a BGZF stream (bytes, or (address, n_bytes)) as it is;
        returns and raises as ingest_bgzf does."""
        res, rd, st, us = _Result(), _Reads(), _IngestStats(), _GunzipStats()
        addr, n, keep = self._host_bytes(blob)
        rc = self._lib.yacrd_engine_ingest_report_bgzf_mem(self._h, addr, n, int(n_threads), float(not_coverage), ctypes.byref(res),
                                                           ctypes.byref(rd), ctypes.byref(st), ctypes.byref(us))
        del keep
        return self._ingested(rc, res, rd, st, us)

    @staticmethod
    def _host_bytes(blob):
        """(address, n_bytes, what keeps them alive) of bytes or of an (address, n_bytes) pair"""
        if isinstance(blob, tuple):
            return int(blob[0]), int(blob[1]), None
        keep = ctypes.create_string_buffer(bytes(blob), len(blob))
        return ctypes.addressof(keep), len(blob), keep

    def _ingested(self, rc, res, rd, st, us=None):
        if rc == E_FALLBACK:
            raise NeedsHostParser(self._lib.yacrd_last_error().decode())
        _check(self._lib, rc)
        R = int(rd.n_reads)
        lengths = np.ctypeslib.as_array(rd.lengths, shape=(R,)).copy() if R else np.zeros(0, np.uint32)
        off = np.ctypeslib.as_array(rd.name_off, shape=(R + 1,)).copy()
        blob = ctypes.string_at(rd.names, int(off[-1])) if R else b""
        names = [blob[int(off[i]):int(off[i + 1])].decode("utf-8", "surrogateescape") for i in range(R)]
        stats = {n: getattr(st, n) for n, _ in _IngestStats._fields_}
        if us is not None:
            stats["inflate"] = {f: getattr(us, f) for f, _ in _GunzipStats._fields_}
        self._lib.yacrd_reads_free(ctypes.byref(rd))
        return _take(self._lib, res), names, lengths, stats

    def _report_table(self, names, lengths, result):
        """(names, lengths, Result) -> a pointer to a yacrd_report_table (None: the resident form) and what keeps its memory
        alive; names: str or bytes, one per read."""
        if names is None and lengths is None and result is None:
            return None, None
        if names is None or lengths is None or result is None:
            raise ValueError("names, lengths and result: all three, or none for the table the last ingest left on the device")
        blobs = [n if isinstance(n, bytes) else n.encode("utf-8", "surrogateescape") for n in names]
        R = len(blobs)
        off = np.zeros(R + 1, np.uint64)
        if blobs:
            off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
        blob = ctypes.create_string_buffer(b"".join(blobs), int(off[-1]) + 1)
        lens = np.ascontiguousarray(lengths, dtype=np.uint32)
        bo = np.ascontiguousarray(result.bad_offsets, dtype=np.uint64)
        br = np.ascontiguousarray(result.bad_regions, dtype=np.uint32).reshape(-1)
        rt = np.ascontiguousarray(result.read_type, dtype=np.uint8)
        if lens.shape != (R,) or bo.shape != (R + 1,) or rt.shape != (R,) or (R and br.size != 2 * int(bo[-1])):
            raise ValueError("the report table's arrays do not fit one another")
        if br.size == 0:
            br = np.zeros(2, np.uint32)
        if R == 0:
            lens, rt = np.zeros(1, np.uint32), np.zeros(1, np.uint8)
        t = _ReportTable(R, off.ctypes.data, ctypes.addressof(blob), lens.ctypes.data, bo.ctypes.data, br.ctypes.data, rt.ctypes.data)
        return ctypes.byref(t), (t, off, blob, lens, bo, br, rt)

    def _report_written(self, rc, st):
        if rc == E_FALLBACK:
            raise NeedsHostParser(self._lib.yacrd_last_error().decode())
        _check(self._lib, rc)
        self.report_write_stats = {n: getattr(st, n) for n, _ in _ReportWriteStats._fields_}
        return self.report_write_stats

    def write_report(self, out_path, names=None, lengths=None, result=None):
        """yacrd_engine_write_report: the .yacrd report of (names, lengths, result) — result: anything with bad_offsets,
        bad_regions and read_type, such as a Result — formatted on the GPU into out_path, byte for byte the host writer's.
        All three None: the RESIDENT form, from the table this engine's last ingest_paf / ingest_text / ingest_report left in
        HBM.  Returns the stats (also self.report_write_stats).  Raises NeedsHostParser, with nothing written, when the table
        or the output is the host writer's (host: yacrd_report_write) or no ingest's table is resident."""
        t, keep = self._report_table(names, lengths, result)
        st = _ReportWriteStats()
        rc = self._lib.yacrd_engine_write_report(self._h, t, os.fsencode(out_path), ctypes.byref(st))
        del keep
        return self._report_written(rc, st)

    def report_text(self, names=None, lengths=None, result=None):
        """yacrd_engine_write_report_mem: the same report as bytes; the stats are in self.report_write_stats."""
        t, keep = self._report_table(names, lengths, result)
        st = _ReportWriteStats()
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._lib.yacrd_engine_write_report_mem(self._h, t, ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(st))
        del keep
        self._report_written(rc, st)
        try:
            return ctypes.string_at(out.value, int(n_out.value)) if n_out.value else b""
        finally:
            self._lib.yacrd_edit_text_free(out)

    def debug_sort_pairs(self, keys, vals, key_bound):
        """yacrd_debug_sort_pairs (tests): (u64 key, u32 value) pairs sorted by key on the device, stable; returns copies."""
        keys = np.array(keys, dtype=np.uint64)
        vals = np.array(vals, dtype=np.uint32)
        _check(self._lib, self._lib.yacrd_debug_sort_pairs(self._h, keys.ctypes.data, vals.ctypes.data, keys.shape[0], int(key_bound)))
        return keys, vals

    def debug_input_csr(self):
        """yacrd_debug_last_input_csr (tests): the input CSR the engine's last call built or staged in its own buffers in HBM,
        as (offsets u64[R+1], intervals u32[I,2], lengths u32[R]); None when that call left none (a _device form, ingest_report,
        trim, a failed call) or a submitted batch is pending."""
        f = self._lib.yacrd_debug_last_input_csr
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p]
        R, I = ctypes.c_uint64(), ctypes.c_uint64()
        rc = f(self._h, ctypes.byref(R), ctypes.byref(I), None, None, None)
        if rc == 1:  # YACRD_EINVAL
            return None
        _check(self._lib, rc)
        off = np.zeros(R.value + 1, dtype=np.uint64)
        iv = np.zeros((I.value, 2), dtype=np.uint32)
        ln = np.zeros(R.value, dtype=np.uint32)
        _check(self._lib, f(self._h, ctypes.byref(R), ctypes.byref(I), off.ctypes.data, iv.ctypes.data, ln.ctypes.data))
        return off, iv, ln

    def debug_counters(self):
        """yacrd_debug_last_counters (tools, tests): the device-side counter block of the last run, by name
        (csrc/device_common.h: struct Counters; the layout is mirrored here and is not part of any ABI)."""
        class _Counters(ctypes.Structure):
            _fields_ = [("n", ctypes.c_uint32 * 16), ("iv", ctypes.c_uint64 * 16), ("rej_small", ctypes.c_uint32),
                        ("rej_med", ctypes.c_uint32), ("rej_big", ctypes.c_uint32), ("region_overflow", ctypes.c_uint32),
                        ("scan_ticket", ctypes.c_uint32), ("ob_unsupported", ctypes.c_uint32), ("prefiltered", ctypes.c_uint32),
                        ("over_med", ctypes.c_uint32), ("fb_med", ctypes.c_uint32 * 2), ("fb_big", ctypes.c_uint32),
                        ("fbq_head", ctypes.c_uint32 * 2), ("fbq_done", ctypes.c_uint32 * 2), ("bs_chunks", ctypes.c_uint32),
                        ("fused_gave_up", ctypes.c_uint32), ("total_regions", ctypes.c_uint64), ("fb_stream", ctypes.c_uint32 * 2),
                        ("_pad", ctypes.c_uint32 * 26),  # (alignas(128): deferred begins a cache line)
                        ("deferred", ctypes.c_uint32), ("deferred_sorted", ctypes.c_uint32), ("deferred_iv", ctypes.c_uint64)]
        c = _Counters()
        self._lib.yacrd_debug_last_counters.restype = ctypes.c_uint64
        self._lib.yacrd_debug_last_counters.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        self._lib.yacrd_debug_last_counters(self._h, ctypes.byref(c), ctypes.sizeof(c))
        out = {}
        for n, _ in _Counters._fields_:
            if n == "_pad":
                continue
            v = getattr(c, n)
            out[n] = list(v) if hasattr(v, "__len__") else int(v)
        return out

    def direct_runs(self):
        """yacrd_debug_direct_runs (tests, tools): runs of this engine whose long launch took its H16 reads by index, beside
        the plan (F_SCREEN_DIRECT; csrc/screen_reg.h: screen_block_rows)."""
        self._lib.yacrd_debug_direct_runs.restype = ctypes.c_uint64
        self._lib.yacrd_debug_direct_runs.argtypes = [ctypes.c_void_p]
        return int(self._lib.yacrd_debug_direct_runs(self._h))

    def big_routes(self):
        """yacrd_debug_big_routes (tests, tools): the last completed run's reads beyond 16 384 intervals by the tier that
        decided them: (device-wide screen, thinned and swept in LDS, entered the segmented sort, handed to the exact kernel).
        A thinned read the LDS sweep rejects, and a read the sort finds degenerate, count under their tier and the last."""
        out = (ctypes.c_uint64 * 4)()
        self._lib.yacrd_debug_big_routes.restype = None
        self._lib.yacrd_debug_big_routes.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._lib.yacrd_debug_big_routes(self._h, out)
        return tuple(int(v) for v in out)

    def debug_seq_window(self, window_bytes):
        """yacrd_debug_seq_window (tests, A/B): the FASTQ and FASTA editors' window.  0: the policy (128 MiB windows where the whole text
        finds no room); 2**64 - 1: never windows; any other value: rounded up to a 32 KiB tile, and every FASTQ or FASTA text longer
        than it is edited window by window (csrc/gpu_seq_edit.hip: run_windows).  The BGZF-in forms take at least 64 KiB and end
        their windows where members end (host.bgzf_window_cuts).  The bytes written do not depend on it."""
        self._lib.yacrd_debug_seq_window.restype = ctypes.c_int
        self._lib.yacrd_debug_seq_window.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        _check(self._lib, self._lib.yacrd_debug_seq_window(self._h, int(window_bytes)))

    def debug_long_min_reads(self, min_reads):
        """yacrd_debug_long_min_reads (tests, A/B): batches of `min_reads` reads and more take the long-batch forms of the plan and
        the follow-on step on this engine (csrc/finish_compact.h: the marks listed, the deferred reads through the filtered exact
        sweep, what it leaves sorted whole — debug_counters()["deferred_sorted"] with F_COUNT_PREFILTERED).  0: every batch;
        2**64 - 1: the default again (400 000 reads, or YACRD_SPLIT_MIN_READS).  The result does not depend on it."""
        self._lib.yacrd_debug_long_min_reads.restype = ctypes.c_int
        self._lib.yacrd_debug_long_min_reads.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        _check(self._lib, self._lib.yacrd_debug_long_min_reads(self._h, int(min_reads)))

    def compute_units(self):
        """yacrd_debug_compute_units (tests): the compute units the engine sizes its resident grids by."""
        self._lib.yacrd_debug_compute_units.restype = ctypes.c_uint64
        self._lib.yacrd_debug_compute_units.argtypes = [ctypes.c_void_p]
        return int(self._lib.yacrd_debug_compute_units(self._h))

    def seq_windows(self):
        """yacrd_debug_seq_windows (tests, tools): what the last sequence edit ran as: its windows (0: the whole text at
        once), the longest carry in bytes, the device bytes of its text ring (BGZF in: with the compressed slot and the member
        slice) and of its output ring."""
        out = (ctypes.c_uint64 * 4)()
        self._lib.yacrd_debug_seq_windows.restype = None
        self._lib.yacrd_debug_seq_windows.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._lib.yacrd_debug_seq_windows(self._h, out)
        return dict(zip(("windows", "max_carry", "text_ring_bytes", "out_ring_bytes"), (int(v) for v in out)))

    def debug_edit_window(self, window_bytes):
        """yacrd_debug_edit_window (tests, A/B): the overlap editor's window.  0: the policy (128 MiB windows where the whole text
        finds no room); 2**64 - 1: never windows; any other value: rounded up to a 32 KiB tile, and every plain overlap text
        longer than it is edited window by window (csrc/gpu_edit.hip: windows_loop).  The resident forms and an edit from the
        parser's mirror take their windows from the text in HBM and hold no text ring; for the BGZF-in forms the window is at
        least 64 KiB and the windows end where members end.  The bytes written do not depend on it."""
        self._lib.yacrd_debug_edit_window.restype = ctypes.c_int
        self._lib.yacrd_debug_edit_window.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        _check(self._lib, self._lib.yacrd_debug_edit_window(self._h, int(window_bytes)))

    def edit_windows(self):
        """yacrd_debug_edit_windows (tests, tools): what the last overlap edit ran as: its windows (0: the whole text at once),
        the farthest a line that began in one window reached into the next, the device bytes of its text ring (BGZF in: with
        the decoder's compressed slot and member slice; from the mirror: 0) and of its output ring."""
        out = (ctypes.c_uint64 * 4)()
        self._lib.yacrd_debug_edit_windows.restype = None
        self._lib.yacrd_debug_edit_windows.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._lib.yacrd_debug_edit_windows(self._h, out)
        return dict(zip(("windows", "max_reach", "text_ring_bytes", "out_ring_bytes"), (int(v) for v in out)))

    def _type_table(self, names, read_type):
        """(names, read_type) -> a yacrd_type_table and what keeps its memory alive; names: str or bytes, one per read."""
        blobs = [n if isinstance(n, bytes) else n.encode("utf-8", "surrogateescape") for n in names]
        off = np.zeros(len(blobs) + 1, np.uint64)
        if blobs:
            off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
        blob = ctypes.create_string_buffer(b"".join(blobs), int(off[-1]) + 1)
        types = np.ascontiguousarray(read_type, dtype=np.uint8)
        if types.shape != (len(blobs),):
            raise ValueError("read_type: one type per name")
        tt = _TypeTable(len(blobs), off.ctypes.data, ctypes.addressof(blob), types.ctypes.data)
        return tt, (off, blob, types)

    def _edited(self, rc, st):
        if rc == E_FALLBACK:
            raise NeedsHostParser(self._lib.yacrd_last_error().decode())
        _check(self._lib, rc)
        self.edit_stats = {n: getattr(st, n) for n, _ in _EditStats._fields_}
        return self.edit_stats

    def edit_overlaps(self, op, src, out_path, names, read_type, fmt=0, n_threads=0):
        """yacrd_engine_edit_overlaps: filter (op 1) / extract (op 2) the overlap file `src` into `out_path` on the GPU, by the
        types of the reads `names`; returns the stats (also self.edit_stats).  Raises NeedsHostParser, with nothing written,
        when the input is the host loop's (host.edit_file)."""
        tt, keep = self._type_table(names, read_type)
        st = _EditStats()
        rc = self._lib.yacrd_engine_edit_overlaps(self._h, int(op), os.fsencode(src), os.fsencode(out_path), int(fmt), int(n_threads),
                                                  ctypes.byref(tt), ctypes.byref(st))
        del keep
        return self._edited(rc, st)

    def edit_overlaps_text(self, op, text, names, read_type, fmt):
        """yacrd_engine_edit_overlaps_mem: the same over `text` (bytes; fmt 1 = PAF, 2 = M4 / MHAP) -> the kept bytes; the
        stats are in self.edit_stats."""
        tt, keep = self._type_table(names, read_type)
        st = _EditStats()
        buf = ctypes.create_string_buffer(bytes(text), len(text) + 1)
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._lib.yacrd_engine_edit_overlaps_mem(self._h, int(op), ctypes.addressof(buf), len(text), int(fmt), ctypes.byref(tt),
                                                      ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(st))
        del keep
        self._edited(rc, st)
        try:
            return ctypes.string_at(out.value, int(n_out.value)) if n_out.value else b""
        finally:
            self._lib.yacrd_edit_text_free(out)

    def edit_overlaps_gzip(self, op, text, names, read_type, fmt, out_path=None):
        """yacrd_engine_edit_overlaps_gzip_mem / _file: filter (op 1) / extract (op 2) the overlap `text` (inflated; bytes or
        anything else with the buffer protocol, which is not copied; fmt 1 = PAF, 2 = M4 / MHAP) with the kept bytes deflated
        on the device where they are packed.  Without out_path -> the BGZF stream (bytes: what gzip() gives for the kept
        bytes); with it the stream is written there and (edit stats, gzip stats) returned.  Both are also in self.edit_stats
        and self.gzip_stats.  Raises NeedsHostParser, with nothing written, when the text is the host loop's."""
        tt, keep = self._type_table(names, read_type)
        st, gs = _EditStats(), _GzipStats()
        buf = np.frombuffer(text, dtype=np.uint8)  # (no copy: a text may be gigabytes)
        n = int(buf.size)
        addr = ctypes.c_void_p(buf.ctypes.data if n else None)
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        if out_path is None:
            rc = self._lib.yacrd_engine_edit_overlaps_gzip_mem(self._h, int(op), addr, n, int(fmt), ctypes.byref(tt),
                                                               ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(gs))
        else:
            rc = self._lib.yacrd_engine_edit_overlaps_gzip_file(self._h, int(op), addr, n, int(fmt), ctypes.byref(tt),
                                                                os.fsencode(out_path), ctypes.byref(st), ctypes.byref(gs))
        del keep, buf
        self._edited(rc, st)
        self.gzip_stats = {f: getattr(gs, f) for f, _ in _GzipStats._fields_}
        if out_path is not None:
            return self.edit_stats, self.gzip_stats
        try:
            return ctypes.string_at(out.value, int(n_out.value))
        finally:
            self._lib.yacrd_edit_text_free(out)

    def edit_overlaps_bgzf(self, op, blob, names, read_type, fmt, out_path=None, gzip_out=True):
        """yacrd_engine_edit_overlaps_bgzf_mem / _file: filter (op 1) / extract (op 2) the COMPRESSED overlap file `blob` (BGZF;
        bytes or anything else with the buffer protocol, which is not copied; fmt 1 = PAF, 2 = M4 / MHAP): it crosses the link
        as it is and is inflated on the device, the host inflates nothing.  gzip_out: the result is edit_overlaps_gzip's for
        the inflated text (one BGZF stream), else edit_overlaps_text's (the kept bytes).  Without out_path -> those bytes; with
        it they are written there and (edit stats, gzip stats) returned.  The stats are also in self.edit_stats,
        self.gzip_stats and self.inflate_stats.  Raises NeedsHostParser, with nothing written, when the text is the host
        loop's, `blob` is not BGZF or holds a member the device decoder does not take."""
        tt, keep = self._type_table(names, read_type)
        st, gs, us = _EditStats(), _GzipStats(), _GunzipStats()
        buf = np.frombuffer(blob, dtype=np.uint8)  # (no copy)
        n = int(buf.size)
        addr = ctypes.c_void_p(buf.ctypes.data if n else None)
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        if out_path is None:
            rc = self._lib.yacrd_engine_edit_overlaps_bgzf_mem(self._h, int(op), addr, n, int(fmt), ctypes.byref(tt), int(bool(gzip_out)),
                                                               ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(gs),
                                                               ctypes.byref(us))
        else:
            rc = self._lib.yacrd_engine_edit_overlaps_bgzf_file(self._h, int(op), addr, n, int(fmt), ctypes.byref(tt), int(bool(gzip_out)),
                                                                os.fsencode(out_path), ctypes.byref(st), ctypes.byref(gs), ctypes.byref(us))
        del keep, buf
        return self._edited_to(rc, st, gs, us, out, n_out, out_path)

    def edit_overlaps_resident(self, op, names, read_type, out_path=None, gzip_out=True):
        """yacrd_engine_edit_overlaps_resident_mem / _file: the same on the overlap text the engine's last successful overlap
        ingest (ingest_paf, ingest_text, ingest_bgzf) left in HBM: nothing goes up (edit_stats["mirror_reused"] == 1).  Returns
        as edit_overlaps_bgzf does.  Raises EngineError — not NeedsHostParser: the caller's logic is wrong — when no overlap
        text is resident."""
        tt, keep = self._type_table(names, read_type)
        st, gs = _EditStats(), _GzipStats()
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        if out_path is None:
            rc = self._lib.yacrd_engine_edit_overlaps_resident_mem(self._h, int(op), ctypes.byref(tt), int(bool(gzip_out)), ctypes.byref(out),
                                                                   ctypes.byref(n_out), ctypes.byref(st), ctypes.byref(gs))
        else:
            rc = self._lib.yacrd_engine_edit_overlaps_resident_file(self._h, int(op), ctypes.byref(tt), int(bool(gzip_out)),
                                                                    os.fsencode(out_path), ctypes.byref(st), ctypes.byref(gs))
        del keep
        return self._edited_to(rc, st, gs, None, out, n_out, out_path)

    def _edited_to(self, rc, st, gs, us, out, n_out, out_path):
        self._edited(rc, st)
        self.gzip_stats = {f: getattr(gs, f) for f, _ in _GzipStats._fields_}
        if us is not None:
            self.inflate_stats = {f: getattr(us, f) for f, _ in _GunzipStats._fields_}
        if out_path is not None:
            return self.edit_stats, self.gzip_stats
        try:
            return ctypes.string_at(out.value, int(n_out.value)) if n_out.value else b""
        finally:
            self._lib.yacrd_edit_text_free(out)

    def _seq_table(self, names, lengths, result):
        """(names, lengths, result) -> a yacrd_report_table for the FASTQ editor; result: what run / ingest_* return, or a
        triple (bad_offsets, bad_regions, read_type)."""
        if isinstance(result, (tuple, list)) and not hasattr(result, "bad_offsets"):
            bo, br, rt = result

            class _R:
                bad_offsets, bad_regions, read_type = bo, br, rt
            result = _R
        if len(names) == 0:  # (nothing to look up: every record is NotBad without a region)
            result = type("_E", (), {"bad_offsets": np.zeros(1, np.uint64), "bad_regions": np.zeros(0, np.uint32),
                                     "read_type": np.zeros(0, np.uint8)})
        return self._report_table(names, lengths, result)

    def _seq_edited(self, rc, st):
        if rc == E_FALLBACK:
            raise NeedsHostParser(self._lib.yacrd_last_error().decode())
        _check(self._lib, rc)
        self.seq_edit_stats = {n: getattr(st, n) for n, _ in _SeqEditStats._fields_}
        return self.seq_edit_stats

    def edit_fastq(self, op, src, out_path, names, lengths, result, n_threads=0):
        """yacrd_engine_edit_fastq: scrubb (op 0) / filter (1) / extract (2) / split (3) the plain FASTQ file `src` into
        `out_path` on the GPU, by the table (names, lengths, result); returns the stats (also self.seq_edit_stats).  Raises
        NeedsHostParser, with nothing written, when the input is the host loop's (host.edit_file)."""
        return self._edit_seq_file("fastq", op, src, out_path, names, lengths, result, n_threads)

    def edit_fastq_text(self, op, text, names, lengths, result):
        """yacrd_engine_edit_fastq_mem: the same over `text` (bytes or anything else with the buffer protocol, which is not
        copied) -> the output's bytes; the stats are in self.seq_edit_stats."""
        return self._edit_seq_text("fastq", op, text, names, lengths, result)

    def edit_fastq_gzip(self, op, text, names, lengths, result, out_path=None):
        """yacrd_engine_edit_fastq_gzip_mem / _file: the same over the inflated FASTQ `text` with the output deflated on the
        device where it is gathered.  Without out_path -> the BGZF stream (bytes: what gzip() gives for edit_fastq_text's
        bytes); with it the stream is written there and (seq edit stats, gzip stats) returned.  Both are also in
        self.seq_edit_stats and self.gzip_stats.  Raises NeedsHostParser, with nothing written, when the text is the host loop's."""
        return self._edit_seq_gzip("fastq", op, text, names, lengths, result, out_path)

    def edit_fasta(self, op, src, out_path, names, lengths, result, n_threads=0):
        """yacrd_engine_edit_fasta: edit_fastq for a plain FASTA file: records of any number of lines, the key the whole name,
        every record that goes out written again 80 bases a line, a cut piece without its description."""
        return self._edit_seq_file("fasta", op, src, out_path, names, lengths, result, n_threads)

    def edit_fasta_text(self, op, text, names, lengths, result):
        """yacrd_engine_edit_fasta_mem: edit_fastq_text for FASTA."""
        return self._edit_seq_text("fasta", op, text, names, lengths, result)

    def edit_fasta_gzip(self, op, text, names, lengths, result, out_path=None):
        """yacrd_engine_edit_fasta_gzip_mem / _file: edit_fastq_gzip for FASTA (what gzip() gives for edit_fasta_text's bytes)."""
        return self._edit_seq_gzip("fasta", op, text, names, lengths, result, out_path)

    def _edit_seq_file(self, fmt, op, src, out_path, names, lengths, result, n_threads):
        t, keep = self._seq_table(names, lengths, result)
        st = _SeqEditStats()
        rc = getattr(self._lib, "yacrd_engine_edit_" + fmt)(self._h, int(op), os.fsencode(src), os.fsencode(out_path), int(n_threads), t,
                                                            ctypes.byref(st))
        del keep
        return self._seq_edited(rc, st)

    def _edit_seq_text(self, fmt, op, text, names, lengths, result):
        t, keep = self._seq_table(names, lengths, result)
        st = _SeqEditStats()
        buf = np.frombuffer(text, dtype=np.uint8)
        n = int(buf.size)
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        rc = getattr(self._lib, "yacrd_engine_edit_%s_mem" % fmt)(self._h, int(op), ctypes.c_void_p(buf.ctypes.data if n else None), n, t,
                                                                  ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(st))
        del keep, buf
        self._seq_edited(rc, st)
        try:
            return ctypes.string_at(out.value, int(n_out.value)) if n_out.value else b""
        finally:
            self._lib.yacrd_edit_text_free(out)

    def edit_fastq_bgzf(self, op, blob, names, lengths, result, out_path=None):
        """yacrd_engine_edit_fastq_bgzf_mem / _file: edit_fastq_gzip over the COMPRESSED file `blob` (BGZF; bytes or anything
        else with the buffer protocol): it crosses the link as it is and is inflated on the device.  The result is
        edit_fastq_gzip's for the inflated text; the inflate's stats are in self.gunzip_stats.  A text of more than a window
        that finds no room whole (or with debug_seq_window set) is inflated and edited window by window, the windows cut where
        members end (host.bgzf_window_cuts; seq_windows() says how the edit ran).  Raises NeedsHostParser, with nothing
        written, also when `blob` is not BGZF or holds a member the device decoder does not take."""
        return self._edit_seq_gzip("fastq", op, blob, names, lengths, result, out_path, bgzf=True)

    def edit_fasta_bgzf(self, op, blob, names, lengths, result, out_path=None):
        """yacrd_engine_edit_fasta_bgzf_mem / _file: edit_fastq_bgzf for FASTA, in windows under the same rule."""
        return self._edit_seq_gzip("fasta", op, blob, names, lengths, result, out_path, bgzf=True)

    def gunzip(self, data):
        """yacrd_engine_gunzip_mem: a BGZF stream (bytes) -> its text (bytes), inflated on the device; the stats are in
        self.gunzip_stats.  Raises NeedsHostParser, with nothing returned, when `data` is not BGZF or holds a member the
        device decoder does not take (host.text_from_file reads those)."""
        buf = np.frombuffer(data, dtype=np.uint8)
        n = int(buf.size)
        st = _GunzipStats()
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._lib.yacrd_engine_gunzip_mem(self._h, ctypes.c_void_p(buf.ctypes.data if n else None), n, ctypes.byref(out), ctypes.byref(n_out),
                                               ctypes.byref(st))
        del buf
        if rc == E_FALLBACK:
            raise NeedsHostParser(self._lib.yacrd_last_error().decode())
        _check(self._lib, rc)
        self.gunzip_stats = {f: getattr(st, f) for f, _ in _GunzipStats._fields_}
        try:
            return ctypes.string_at(out.value, int(n_out.value)) if n_out.value else b""
        finally:
            self._lib.yacrd_edit_text_free(out)

    def gunzip_stream(self, data):
        """yacrd_engine_gunzip_stream_mem: ONE plain gzip member (bytes) -> its text (bytes), inflated on the device from block
        starts found in parallel; the stats are in self.gunzip_stream_stats.  Raises NeedsHostParser, with nothing returned,
        when `data` is not one gzip member (BGZF and concatenated members among them) or its payload is one the device decoder
        does not take (host.text_from_file reads those)."""
        buf = np.frombuffer(data, dtype=np.uint8)
        n = int(buf.size)
        st = _GunzipStreamStats()
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._lib.yacrd_engine_gunzip_stream_mem(self._h, ctypes.c_void_p(buf.ctypes.data if n else None), n, ctypes.byref(out),
                                                      ctypes.byref(n_out), ctypes.byref(st))
        del buf
        if rc == E_FALLBACK:
            raise NeedsHostParser(self._lib.yacrd_last_error().decode())
        _check(self._lib, rc)
        self.gunzip_stream_stats = {f: getattr(st, f) for f, _ in _GunzipStreamStats._fields_}
        try:
            return ctypes.string_at(out.value, int(n_out.value)) if n_out.value else b""
        finally:
            self._lib.yacrd_edit_text_free(out)

    def debug_gunzip_chunk(self, n_bytes):
        """yacrd_debug_gunzip_chunk (tests, A/B): gunzip_stream looks for a block start once per `n_bytes` of compressed payload
        (at least 1024; 0: YACRD_GUNZIP_CHUNK or the default, 32 KiB).  The text does not depend on it."""
        self._lib.yacrd_debug_gunzip_chunk.restype = ctypes.c_int
        self._lib.yacrd_debug_gunzip_chunk.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _check(self._lib, self._lib.yacrd_debug_gunzip_chunk(self._h, int(n_bytes)))

    def edit_fastq_gz(self, op, blob, names, lengths, result, out_path=None):
        """yacrd_engine_edit_fastq_gz_mem / _file: edit_fastq_gzip over ONE plain gzip member `blob` (bytes or anything else
        with the buffer protocol): it crosses the link as it is and is inflated on the device (gunzip_stream's steps).  The
        result is edit_fastq_gzip's for the inflated text; the inflate's stats are in self.gunzip_stream_stats.  The
        whole-text run only.  Raises NeedsHostParser, with nothing written, also when `blob` is not one gzip member or its
        payload is one the device decoder does not take."""
        return self._edit_seq_gzip("fastq", op, blob, names, lengths, result, out_path, gz=True)

    def edit_fasta_gz(self, op, blob, names, lengths, result, out_path=None):
        """yacrd_engine_edit_fasta_gz_mem / _file: edit_fastq_gz for FASTA."""
        return self._edit_seq_gzip("fasta", op, blob, names, lengths, result, out_path, gz=True)

    def _edit_seq_gzip(self, fmt, op, text, names, lengths, result, out_path, bgzf=False, gz=False):
        t, keep = self._seq_table(names, lengths, result)
        st, gs, us = _SeqEditStats(), _GzipStats(), _GunzipStreamStats() if gz else _GunzipStats()
        more = (ctypes.byref(us),) if bgzf or gz else ()
        kind = "bgzf" if bgzf else "gz" if gz else "gzip"
        buf = np.frombuffer(text, dtype=np.uint8)
        n = int(buf.size)
        addr = ctypes.c_void_p(buf.ctypes.data if n else None)
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        if out_path is None:
            rc = getattr(self._lib, "yacrd_engine_edit_%s_%s_mem" % (fmt, kind))(self._h, int(op), addr, n, t, ctypes.byref(out), ctypes.byref(n_out),
                                                                                 ctypes.byref(st), ctypes.byref(gs), *more)
        else:
            rc = getattr(self._lib, "yacrd_engine_edit_%s_%s_file" % (fmt, kind))(self._h, int(op), addr, n, t, os.fsencode(out_path), ctypes.byref(st),
                                                                                  ctypes.byref(gs), *more)
        del keep, buf
        self._seq_edited(rc, st)
        if bgzf:
            self.gunzip_stats = {f: getattr(us, f) for f, _ in _GunzipStats._fields_}
        if gz:
            self.gunzip_stream_stats = {f: getattr(us, f) for f, _ in _GunzipStreamStats._fields_}
        self.gzip_stats = {f: getattr(gs, f) for f, _ in _GzipStats._fields_}
        if out_path is not None:
            return self.seq_edit_stats, self.gzip_stats
        try:
            return ctypes.string_at(out.value, int(n_out.value))
        finally:
            self._lib.yacrd_edit_text_free(out)

    def gzip(self, data):
        """yacrd_engine_gzip_mem: `data` (bytes) -> one BGZF stream (bytes), compressed on the device; the stats are in
        self.gzip_stats."""
        data = bytes(data)
        st = _GzipStats()
        out, n_out = ctypes.c_void_p(), ctypes.c_uint64()
        buf = ctypes.create_string_buffer(data, len(data) + 1)
        _check(self._lib, self._lib.yacrd_engine_gzip_mem(self._h, ctypes.addressof(buf), len(data), ctypes.byref(out), ctypes.byref(n_out),
                                                          ctypes.byref(st)))
        self.gzip_stats = {f: getattr(st, f) for f, _ in _GzipStats._fields_}
        try:
            return ctypes.string_at(out.value, int(n_out.value))
        finally:
            self._lib.yacrd_edit_text_free(out)

    def gzip_writer(self, out_path, segment_bytes=0, n_buffers=0):
        """A GzipWriter over this engine (yacrd_gzip_writer_open)."""
        return GzipWriter(self, out_path, segment_bytes, n_buffers)

    def trim(self):
        """yacrd_engine_trim: give the device parser's and the overlap editor's buffers back."""
        _check(self._lib, self._lib.yacrd_engine_trim(self._h))

    def fetch(self):
        res = _Result()
        _check(self._lib, self._lib.yacrd_engine_fetch(self._h, ctypes.byref(res)))
        return _take(self._lib, res)

    def timing(self):
        t = _Timing()
        _check(self._lib, self._lib.yacrd_engine_last_timing(self._h, ctypes.byref(t)))
        out = {}
        for n, _ in _Timing._fields_:
            v = getattr(t, n)
            out[n] = list(v) if n.startswith("class_") else v
        return out

    def event_overhead_ms(self):
        """Elapsed time of an empty HIP-event bracket on the engine's stream."""
        ms = ctypes.c_float()
        _check(self._lib, self._lib.yacrd_engine_event_overhead(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def timing_total(self, reset=False):
        """(sums over the runs since the last reset, number of runs)."""
        t = _Timing()
        n = ctypes.c_uint64()
        _check(self._lib, self._lib.yacrd_engine_timing_total(self._h, ctypes.byref(t),
                                                              ctypes.byref(n), 1 if reset else 0))
        out = {}
        for name, _ in _Timing._fields_:
            v = getattr(t, name)
            out[name] = list(v) if name.startswith("class_") else v
        return out, int(n.value)

    def submit(self, offsets, intervals, lengths, coverage, not_coverage):
        """run() without the final wait (yacrd_engine_submit); the arrays must stay alive and
        unchanged until collect().  Pass PinnedArray.array views for direct DMA."""
        n_reads = offsets.shape[0] - 1
        self._keep = (offsets, intervals, lengths)
        _check(self._lib, self._lib.yacrd_engine_submit(
            self._h, _ptr(offsets, ctypes.c_uint64), _ptr(intervals.reshape(-1), ctypes.c_uint32),
            _ptr(lengths, ctypes.c_uint32), n_reads, min(int(coverage), 0xFFFFFFFF),
            float(not_coverage)))

    def collect(self):
        res = _Result()
        _check(self._lib, self._lib.yacrd_engine_collect(self._h, ctypes.byref(res)))
        self._keep = None
        return _take(self._lib, res)

    def classify(self, bad_offsets, bad_regions, lengths, not_coverage):
        bad_offsets = np.ascontiguousarray(bad_offsets, dtype=np.uint64)
        bad_regions = np.ascontiguousarray(bad_regions, dtype=np.uint32).reshape(-1)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        n_reads = lengths.shape[0]
        out = np.zeros(max(n_reads, 1), dtype=np.uint8)
        if bad_regions.size == 0:
            bad_regions = np.zeros(2, dtype=np.uint32)
        _check(self._lib, self._lib.yacrd_engine_classify(
            self._h, _ptr(bad_offsets, ctypes.c_uint64), _ptr(bad_regions, ctypes.c_uint32),
            _ptr(lengths, ctypes.c_uint32), n_reads, float(not_coverage),
            _ptr(out, ctypes.c_uint8)))
        return out[:n_reads]


class GzipWriter:
    """yacrd_gzip_writer: bytes arrive through write(), leave as a BGZF file compressed on the device.  As a context
    manager it closes on a clean exit and aborts (nothing is left at out_path) on an exception."""

    def __init__(self, engine, out_path, segment_bytes=0, n_buffers=0):
        self._lib = engine._lib
        self._engine = engine
        self._h = ctypes.c_void_p()
        self.stats = None
        _check(self._lib, self._lib.yacrd_gzip_writer_open(engine._h, os.fsencode(out_path), int(segment_bytes), int(n_buffers),
                                                           ctypes.byref(self._h)))

    def write(self, data):
        data = bytes(data)
        if not self._h:
            raise EngineError("the gzip writer is closed")
        _check(self._lib, self._lib.yacrd_gzip_writer_write(self._h, data, len(data)))
        return len(data)

    def sink(self):
        """A ByteSink (yacrd_gzip_writer_sink) for host.edit_file_to; valid while the writer is open."""
        s = ByteSink()
        _check(self._lib, self._lib.yacrd_gzip_writer_sink(self._h, ctypes.byref(s)))
        return s

    def close(self):
        if not self._h:
            return self.stats
        h, self._h = self._h, ctypes.c_void_p()
        st = _GzipStats()
        _check(self._lib, self._lib.yacrd_gzip_writer_close(h, ctypes.byref(st)))
        self.stats = {f: getattr(st, f) for f, _ in _GzipStats._fields_}
        return self.stats

    def abort(self):
        if self._h:
            h, self._h = self._h, ctypes.c_void_p()
            self._lib.yacrd_gzip_writer_abort(h)

    def __del__(self):  # (a writer that was dropped: the engine gets its buffers back, nothing is left beside out_path)
        try:
            self.abort()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()
        return False


class PinnedArray:
    """A numpy array over page-locked host memory (yacrd_pinned_alloc): the engine moves it over
    PCIe by direct DMA.  Keep the object alive while `array` is in use."""

    def __init__(self, shape, dtype):
        self._lib = load_library()
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        self._p = self._lib.yacrd_pinned_alloc(max(n, 1))
        if not self._p:
            raise EngineError("yacrd_pinned_alloc(%d) failed" % n)
        buf = (ctypes.c_char * max(n, 1)).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    @classmethod
    def copy_of(cls, a):
        a = np.ascontiguousarray(a)
        p = cls(a.shape, a.dtype)
        p.array[...] = a
        return p

    def close(self):
        if self._p:
            self.array = None
            self._lib.yacrd_pinned_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream:
    """yacrd_stream: overlap records go to HBM from pinned buffers while they are produced; finish()
    builds the CSR on the GPU and runs the engine on it."""

    def __init__(self, engine, chunk_records=0, n_buffers=0):
        self._lib = load_library()
        self._engine = engine
        self._h = ctypes.c_void_p()
        _check(self._lib, self._lib.yacrd_stream_open(engine._h, chunk_records, n_buffers,
                                                      ctypes.byref(self._h)))

    def sink(self):
        """A RecSink for host.ingest_stream (keep this Stream alive while it is in use)."""
        s = RecSink()
        _check(self._lib, self._lib.yacrd_stream_sink(self._h, ctypes.byref(s)))
        return s

    def push(self, recs):
        """Copy an OVL_REC_DTYPE array into stream buffers (tests; the parser fills them in place)."""
        recs = np.ascontiguousarray(recs, dtype=OVL_REC_DTYPE)
        at = 0
        while at < len(recs):
            buf = ctypes.POINTER(OvlRec)()
            cap = ctypes.c_uint64()
            _check(self._lib, self._lib.yacrd_stream_acquire(self._h, ctypes.byref(buf), ctypes.byref(cap)))
            n = min(int(cap.value), len(recs) - at)
            ctypes.memmove(buf, recs[at:at + n].ctypes.data, n * OVL_REC_DTYPE.itemsize)
            _check(self._lib, self._lib.yacrd_stream_commit(self._h, buf, n))
            at += n

    def finish(self, handle_map, lengths, coverage, not_coverage):
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if handle_map is not None:
            handle_map = np.ascontiguousarray(handle_map, dtype=np.uint32)
        res = _Result()
        _check(self._lib, self._lib.yacrd_stream_finish(
            self._h, _ptr(handle_map, ctypes.c_uint32) if handle_map is not None and handle_map.size else None,
            0 if handle_map is None else handle_map.shape[0],
            _ptr(lengths, ctypes.c_uint32) if lengths.size else None, lengths.shape[0],
            min(int(coverage), 0xFFFFFFFF), float(not_coverage), ctypes.byref(res)))
        return _take(self._lib, res)

    def reset(self):
        """Discard every record committed so far (after a failed ingest)."""
        _check(self._lib, self._lib.yacrd_stream_reset(self._h))

    def stats(self):
        st = _StreamStats()
        _check(self._lib, self._lib.yacrd_stream_last_stats(self._h, ctypes.byref(st)))
        return {n: getattr(st, n) for n, _ in _StreamStats._fields_}

    def close(self):
        if self._h:
            self._lib.yacrd_stream_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


HANDLE_ELSEWHERE = 0xFFFFFFFE


def stream_device_of(handle, n_devices):
    """The device a read belongs to in a StreamGroup (yacrd_stream_device_of: handle mod N).  Loads the
    library only: no GPU needed."""
    return int(load_library().yacrd_stream_device_of(int(handle), int(n_devices)))


class StreamGroup:
    """yacrd_stream_group: one yacrd_stream per engine; the sink routes every record to the device(s) of its two
    reads while the parser runs, finish() builds one CSR per device, runs them side by side and merges the
    results into first-appearance order."""

    def __init__(self, engines, chunk_records=0, n_buffers=0):
        self._lib = load_library()
        self._engines = list(engines)
        arr = (ctypes.c_void_p * len(self._engines))(*[e._h for e in self._engines])
        self._h = ctypes.c_void_p()
        _check(self._lib, self._lib.yacrd_stream_group_open(arr, len(self._engines), chunk_records, n_buffers,
                                                            ctypes.byref(self._h)))
        self._sink = None

    def sink(self):
        s = RecSink()
        _check(self._lib, self._lib.yacrd_stream_group_sink(self._h, ctypes.byref(s)))
        return s

    def push(self, recs):
        """Copy an OVL_REC_DTYPE array through the group's sink (tests; the parser fills buffers in place)."""
        recs = np.ascontiguousarray(recs, dtype=OVL_REC_DTYPE)
        if self._sink is None:
            self._sink = self.sink()
        sink = self._sink
        at = 0
        while at < len(recs):
            buf = ctypes.POINTER(OvlRec)()
            cap = ctypes.c_uint64()
            rc = sink.acquire(sink.ctx, ctypes.byref(buf), ctypes.byref(cap))
            _check(self._lib, rc)
            n = min(int(cap.value), len(recs) - at)
            ctypes.memmove(buf, recs[at:at + n].ctypes.data, n * OVL_REC_DTYPE.itemsize)
            _check(self._lib, sink.commit(sink.ctx, buf, n))
            at += n

    def finish(self, handle_map, lengths, coverage, not_coverage):
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if handle_map is not None:
            handle_map = np.ascontiguousarray(handle_map, dtype=np.uint32)
        res = _Result()
        _check(self._lib, self._lib.yacrd_stream_group_finish(
            self._h, _ptr(handle_map, ctypes.c_uint32) if handle_map is not None and handle_map.size else None,
            0 if handle_map is None else handle_map.shape[0],
            _ptr(lengths, ctypes.c_uint32) if lengths.size else None, lengths.shape[0],
            min(int(coverage), 0xFFFFFFFF), float(not_coverage), ctypes.byref(res)))
        return _take(self._lib, res)

    def reset(self):
        _check(self._lib, self._lib.yacrd_stream_group_reset(self._h))

    def stats(self, index):
        st = _StreamStats()
        owned = ctypes.c_uint64()
        _check(self._lib, self._lib.yacrd_stream_group_last_stats(self._h, index, ctypes.byref(st), ctypes.byref(owned)))
        d = {n: getattr(st, n) for n, _ in _StreamStats._fields_}
        d["reads_owned"] = int(owned.value)
        return d

    def close(self):
        if self._h:
            self._lib.yacrd_stream_group_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
