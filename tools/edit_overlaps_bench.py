#!/usr/bin/env python3
"""tools/edit_overlaps_bench.py [--reads R] [--overlaps O] [--runs K] [--op filter|extract] [--json PATH]
filter / extract on an OVERLAP file, host loop against device editor, on a synthetic PAF in /dev/shm (output there too);
K timed runs of each after one warm-up:
  (a) host     yacrd_edit_file: the one-thread loop (seconds, GB/s of input)
  (b) moved    yacrd_engine_edit_overlaps, the text moved to HBM (warm buffers), with text_ms / kernel_ms / out_ms
  (c) reused   the same from the mirror the device parser left in HBM
  (d) floor    yacrd_ingest_stats.text_ms of the device parser on the file: what moving the text in costs by itself
Every output is compared with the host loop's.  One JSON line (appended to --json when given)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yacrd_amd  # noqa: E402
from yacrd_amd import host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=50_000)
ap.add_argument("--overlaps", type=int, default=5_000_000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--op", default="filter")
ap.add_argument("--json", default=None)
a = ap.parse_args()
op = {"filter": host.OP_FILTER, "extract": host.OP_EXTRACT}[a.op]
d = os.environ.get("YACRD_EDIT_BENCH_DIR", "/dev/shm")
tag = os.path.join(d, "yacrd_eob_%d_" % os.getpid())
paf, want, got = tag + "in.paf", tag + "host.paf", tag + "dev.paf"


def same(x, y):
    with open(x, "rb") as fx, open(y, "rb") as fy:
        while True:
            p, q = fx.read(1 << 24), fy.read(1 << 24)
            if p != q:
                return False
            if not p:
                return True


def fresh(path):
    if os.path.exists(path):
        os.remove(path)  # (or the open's truncation frees the last run's pages inside the timed region)


try:
    host.synth_paf(host.SYNTH_SEQUEL, a.reads, a.overlaps, 20241108 + 5, paf)
    size = os.path.getsize(paf)
    with yacrd_amd.Engine(device_id=0) as e:
        floor = []
        for k in range(a.runs + 1):
            res, names, lengths, st = e.ingest_paf(paf, 3, 0.4)
            if k:
                floor.append(st["text_ms"])
        types = res.read_type
        hs = []
        for k in range(a.runs + 1):
            fresh(want)
            t0 = time.perf_counter()
            host.edit_file(op, paf, want, names, lengths, res.bad_offsets, res.bad_regions, types, n_threads=1)
            if k:
                hs.append(time.perf_counter() - t0)

        def device(reuse):
            rows = []
            for k in range(a.runs + 1):
                if not reuse:
                    e.ingest_text(b"", 3, 0.4)  # (any other parse: the mirror no longer holds the file)
                fresh(got)
                t0 = time.perf_counter()
                s = e.edit_overlaps(op, paf, got, names, types)
                dt = time.perf_counter() - t0
                assert s["mirror_reused"] == (1 if reuse else 0), s
                assert same(want, got), "device bytes differ from the host loop's"
                if k:
                    rows.append({"s": round(dt, 4), "GBps": round(size / dt / 1e9, 2), **{n: round(s[n], 2) for n in ("text_ms", "table_ms", "kernel_ms", "out_ms")}})
            return rows
        reused = device(True)
        moved = device(False)
        e.trim()
    row = {"reads": a.reads, "overlaps": a.overlaps, "op": a.op, "text_bytes": size, "kept_bytes": os.path.getsize(want),
           "host_loop": [{"s": round(x, 3), "GBps": round(size / x / 1e9, 3)} for x in hs],
           "device_text_moved": moved, "device_mirror_reused": reused, "parser_text_ms": [round(x, 2) for x in floor]}
    line = json.dumps(row)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")
finally:
    for x in (paf, want, got):
        if os.path.exists(x):
            os.remove(x)
