#!/usr/bin/env python3
"""tools/report_write_bench.py [--runs K] [--large-overlaps O] [--sizes small,large] [--json PATH]
Writing the `.yacrd` report: host writer against device writer.  The table comes from an engine run over yacrd_synth_csr with
the names read_<i>, at the two sizes of tools/report_read_bench.py:
  small   BASELINE.json configs[1]: 100 k reads / 5 M overlaps (ont)
  large   configs[4]-shaped: 5 M reads (sequel; --large-overlaps, default 100 M: the report's size follows the reads)
Files go to /dev/shm (YACRD_REPORT_BENCH_DIR).  After one warm-up of each, K timed runs of
  (a) host      yacrd_report_write (the parent commit's, unchanged)
  (b) table     yacrd_engine_write_report with the table's seven host arrays, on a warm engine
  (c) resident  yacrd_engine_write_report(NULL) right after yacrd_engine_ingest_report of (a)'s file (the ingest is not timed)
  (d) floor     one thread's pwrite of the same bytes from memory into a new file
The bytes of (b) and (c) are compared with (a)'s BEFORE any time is taken.  The verdict sets the SLOWEST warm (b) and (c)
against the FASTEST (a).  JSON: one object (written to --json when given)."""
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


def read_file(path):
    with open(path, "rb") as f:
        return f.read()


out = {"tool": "report_write_bench", "not_coverage": N, "runs": a.runs, "sizes": {}}
for size in a.sizes.split(","):
    profile, R, O, cov, seed = SIZES[size]
    paths = [os.path.join(d, "yacrd_rwb_%d_%s_%s.yacrd" % (os.getpid(), size, k)) for k in "abcd"]
    pa, pb, pc, pd = paths
    try:
        off, iv, lens = host.synth_csr(profile, R, O, seed)
        with yacrd_amd.Engine(device_id=0) as e:
            res = e.run(off, iv, lens, cov, N)
        del off, iv
        names = np.char.add("read_", np.arange(R).astype(str))
        blob = "".join(names.tolist()).encode()
        name_off = np.zeros(R + 1, np.uint64)
        np.cumsum(np.char.str_len(names), out=name_off[1:])
        del names
        br = np.ascontiguousarray(res.bad_regions, np.uint32).reshape(-1)
        if br.size == 0:
            br = np.zeros(2, np.uint32)
        keep = ctypes.create_string_buffer(blob, len(blob) + 1)
        view = host._View(R, 0, 0, None, None, lens.ctypes.data_as(u32p), name_off.ctypes.data_as(u64p),
                          ctypes.cast(keep, ctypes.POINTER(ctypes.c_char)))
        table = eng._ReportTable(R, name_off.ctypes.data, ctypes.addressof(keep), lens.ctypes.data, res.bad_offsets.ctypes.data,
                                 br.ctypes.data, res.read_type.ctypes.data)

        def host_run():
            t0 = time.perf_counter()
            host._check(hl, hl.yacrd_report_write(pa.encode(), ctypes.byref(view), res.bad_offsets.ctypes.data_as(u64p), br.ctypes.data_as(u32p),
                                                  res.read_type.ctypes.data_as(u8p)))
            return time.perf_counter() - t0

        def device_run(e, path, t):
            st = eng._ReportWriteStats()
            t0 = time.perf_counter()
            rc = el.yacrd_engine_write_report(e._h, t, path.encode(), ctypes.byref(st))
            dt = time.perf_counter() - t0
            eng._check(el, rc)
            return dt, {n: getattr(st, n) for n, _ in eng._ReportWriteStats._fields_}

        def ingest(e):
            r2, rd, ist = eng._Result(), eng._Reads(), eng._IngestStats()
            eng._check(el, el.yacrd_engine_ingest_report(e._h, pa.encode(), 0, N, ctypes.byref(r2), ctypes.byref(rd), ctypes.byref(ist)))
            el.yacrd_reads_free(ctypes.byref(rd))
            el.yacrd_result_free(ctypes.byref(r2))

        host_run()  # warm-up
        want = read_file(pa)
        with yacrd_amd.Engine(device_id=0) as e:
            # the bytes first: (b), then (c) — whose types are those of the ingest's classify with the same N: the file's
            device_run(e, pb, ctypes.byref(table))  # (also the warm-up: buffers, code objects, pinned memory)
            if read_file(pb) != want:
                sys.exit("%s: the table form's bytes differ from the host writer's" % size)
            ingest(e)
            device_run(e, pc, None)
            if read_file(pc) != want:
                sys.exit("%s: the resident form's bytes differ from the host writer's" % size)
            host_s = [host_run() for _ in range(a.runs)]
            tab = [device_run(e, pb, ctypes.byref(table)) for _ in range(a.runs)]
            resid = []
            for _ in range(a.runs):
                ingest(e)
                resid.append(device_run(e, pc, None))
            if read_file(pb) != want or read_file(pc) != want:
                sys.exit("%s: a timed run's bytes differ from the host writer's" % size)
        floor_s = []
        for _ in range(a.runs + 1):
            if os.path.exists(pd):
                os.remove(pd)
            t0 = time.perf_counter()
            fd = os.open(pd, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            done = 0
            mv = memoryview(want)
            while done < len(want):
                done += os.pwrite(fd, mv[done:done + (64 << 20)], done)
            os.close(fd)
            floor_s.append(time.perf_counter() - t0)
        floor_s = floor_s[1:]
        tab_s, res_s = [x[0] for x in tab], [x[0] for x in resid]
        out["sizes"][size] = {
            "reads": R, "overlaps": O, "report_bytes": len(want), "regions": int(res.bad_offsets[-1]), "bytes_equal_checked_first": True,
            "a_host_s": host_s, "b_table_warm_s": tab_s, "c_resident_s": res_s, "d_floor_pwrite_s": floor_s,
            "b_last_stats": tab[-1][1], "c_last_stats": resid[-1][1],
            "b_speedup_slowest_vs_fastest_host": min(host_s) / max(tab_s), "c_speedup_slowest_vs_fastest_host": min(host_s) / max(res_s),
            "b_faster": max(tab_s) < min(host_s), "c_faster": max(res_s) < min(host_s),
        }
    finally:
        for p in paths:
            if os.path.exists(p):
                os.remove(p)
line = json.dumps(out)
print(line)
if a.json:
    with open(a.json, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
