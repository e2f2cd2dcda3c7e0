#!/usr/bin/env python3
"""tools/report_read_bench.py [--runs K] [--large-overlaps O] [--sizes small,large] [--json PATH]
Reading a `.yacrd` report back (FromReport, src/stack.rs:176-257): host reader against device reader.  The report is written
by the project's own writer (yacrd_report_write) from an engine run over yacrd_synth_csr, in /dev/shm, at two sizes:
  small   BASELINE.json configs[1]: 100 k reads / 5 M overlaps (ont)
  large   configs[4]-shaped: 5 M reads (sequel; --large-overlaps, default 100 M: the report's size follows the reads)
After one warm-up of each, K timed runs of
  (a) host    yacrd_report_read + yacrd_report_get + yacrd_engine_classify (the host reader is the parent commit's, unchanged)
  (b) device  yacrd_engine_ingest_report — `cold`: the first call of a fresh engine (buffers allocated, code objects loaded),
              `warm`: calls into the engine's warm buffers
  (c) floor   text_ms of the warm device runs: what moving the text to HBM and counting its lines costs by itself
Every array of (b) — names, name_off, lengths, bad_offsets, bad_regions, read_type — is compared with (a) before anything is
reported.  The verdict sets the SLOWEST warm (b) against the FASTEST (a).  JSON: one object (written to --json when given)."""
import argparse, ctypes, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yacrd_amd  # noqa: E402
from yacrd_amd import engine as eng, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--large-overlaps", type=int, default=100_000_000)
ap.add_argument("--sizes", default="small,large")
ap.add_argument("--json", default=None)
a = ap.parse_args()
SIZES = {"small": (host.SYNTH_ONT, 100_000, 5_000_000, 4, 20241108 + 2),
         "large": (host.SYNTH_SEQUEL, 5_000_000, a.large_overlaps, 3, 20241108 + 5)}
N = 0.4
d = os.environ.get("YACRD_REPORT_BENCH_DIR", "/dev/shm")
hl, el = host.load_library(), yacrd_amd.load_library()
u64p, u32p, u8p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint8))


def write_report(path, profile, R, O, cov, seed):
    off, iv, lens = host.synth_csr(profile, R, O, seed)
    with yacrd_amd.Engine(device_id=0) as e:
        res = e.run(off, iv, lens, cov, N)
    names = np.char.add("read_", np.arange(R).astype(str))
    blob = "".join(names.tolist()).encode()
    name_off = np.zeros(R + 1, np.uint64)
    np.cumsum(np.char.str_len(names), out=name_off[1:])
    view = host._View(R, 0, 0, None, None, lens.ctypes.data_as(u32p), name_off.ctypes.data_as(u64p),
                      ctypes.cast(ctypes.c_char_p(blob), ctypes.POINTER(ctypes.c_char)))
    br = np.ascontiguousarray(res.bad_regions, np.uint32).reshape(-1)
    if br.size == 0:
        br = np.zeros(2, np.uint32)
    host._check(hl, hl.yacrd_report_write(path.encode(), ctypes.byref(view), res.bad_offsets.ctypes.data_as(u64p), br.ctypes.data_as(u32p),
                                          res.read_type.ctypes.data_as(u8p)))


def host_run(e, path):
    """(a): seconds, and the arrays (copied out behind the clock)"""
    t0 = time.perf_counter()
    h = ctypes.c_void_p()
    host._check(hl, hl.yacrd_report_read(path.encode(), ctypes.byref(h)))
    v = host._BadParts()
    host._check(hl, hl.yacrd_report_get(h, ctypes.byref(v)))
    R = int(v.n_reads)
    types = np.zeros(R + 1, np.uint8)
    eng._check(el, el.yacrd_engine_classify(e._h, v.bad_offsets, v.bad_regions, v.lengths, R, N, types.ctypes.data_as(u8p)))
    dt = time.perf_counter() - t0
    off = np.ctypeslib.as_array(v.name_off, shape=(R + 1,)).copy()
    bo = np.ctypeslib.as_array(v.bad_offsets, shape=(R + 1,)).copy()
    G = int(bo[-1])
    arrays = (ctypes.string_at(v.names, int(off[-1])), off, np.ctypeslib.as_array(v.lengths, shape=(R,)).copy(), bo,
              np.ctypeslib.as_array(v.bad_regions, shape=(2 * G,)).copy() if G else np.zeros(0, np.uint32), types[:R].copy())
    hl.yacrd_report_free(h)
    return dt, arrays


def device_run(e, path):
    """(b): seconds, the stats, and the arrays"""
    res, rd, st = eng._Result(), eng._Reads(), eng._IngestStats()
    t0 = time.perf_counter()
    rc = el.yacrd_engine_ingest_report(e._h, path.encode(), 0, N, ctypes.byref(res), ctypes.byref(rd), ctypes.byref(st))
    dt = time.perf_counter() - t0
    eng._check(el, rc)
    R, G = int(rd.n_reads), int(res.n_regions)
    off = np.ctypeslib.as_array(rd.name_off, shape=(R + 1,)).copy()
    arrays = (ctypes.string_at(rd.names, int(off[-1])), off, np.ctypeslib.as_array(rd.lengths, shape=(R,)).copy(),
              np.ctypeslib.as_array(res.bad_offsets, shape=(R + 1,)).copy(),
              np.ctypeslib.as_array(res.bad_regions, shape=(2 * G,)).copy() if G else np.zeros(0, np.uint32),
              np.ctypeslib.as_array(res.read_type, shape=(R,)).copy())
    el.yacrd_reads_free(ctypes.byref(rd))
    el.yacrd_result_free(ctypes.byref(res))
    return dt, {n: getattr(st, n) for n, _ in eng._IngestStats._fields_}, arrays


def same(x, y):
    return x[0] == y[0] and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))


out = {"tool": "report_read_bench", "not_coverage": N, "runs": a.runs, "sizes": {}}
for size in a.sizes.split(","):
    profile, R, O, cov, seed = SIZES[size]
    path = os.path.join(d, "yacrd_rrb_%d_%s.yacrd" % (os.getpid(), size))
    try:
        write_report(path, profile, R, O, cov, seed)
        nbytes = os.path.getsize(path)
        with yacrd_amd.Engine(device_id=0) as e:
            _, want = host_run(e, path)  # warm-up (page cache, the classify kernel's code object)
            host_s = [host_run(e, path)[0] for _ in range(a.runs)]
        cold_s = []
        for _ in range(a.runs):  # cold: a fresh engine's first call
            with yacrd_amd.Engine(device_id=0) as e:
                dt, _, got = device_run(e, path)
                if not same(got, want):
                    sys.exit("%s: the device reader's arrays differ from the host reader's (cold)" % size)
                cold_s.append(dt)
        warm_s, floor_ms, stats = [], [], None
        with yacrd_amd.Engine(device_id=0) as e:
            device_run(e, path)
            for _ in range(a.runs):
                dt, stats, got = device_run(e, path)
                if not same(got, want):
                    sys.exit("%s: the device reader's arrays differ from the host reader's (warm)" % size)
                warm_s.append(dt)
                floor_ms.append(stats["text_ms"])
        out["sizes"][size] = {
            "reads": R, "overlaps": O, "report_bytes": nbytes, "lines": int(stats["n_records"]), "regions": int(want[3][-1]),
            "a_host_s": host_s, "b_device_cold_s": cold_s, "b_device_warm_s": warm_s, "c_floor_text_ms": floor_ms,
            "last_warm_stats": stats,
            "host_GBps_min_max": [nbytes / max(host_s) / 1e9, nbytes / min(host_s) / 1e9],
            "device_warm_GBps_min_max": [nbytes / max(warm_s) / 1e9, nbytes / min(warm_s) / 1e9],
            "speedup_slowest_warm_device_vs_fastest_host": min(host_s) / max(warm_s),
            "device_faster": max(warm_s) < min(host_s),
            "arrays_equal": True,
        }
    finally:
        if os.path.exists(path):
            os.remove(path)
line = json.dumps(out)
print(line)
if a.json:
    with open(a.json, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
