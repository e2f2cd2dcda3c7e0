#!/usr/bin/env python3
"""Device inflate, the primitive: Engine.gunzip on the BGZF of the synthetic Sequel FASTQ that tools/edit_fastq_bench.py writes
(50 000 reads: 1 020 895 402 bytes) — the kernel alone (device events) and the whole call — against the host's member-parallel
inflate (host.text_from_file on 16 CPUs) in the same run: K runs of each after a warm-up, every output compared with the
FASTQ.  Writes profiles/gpu_inflate.json (the "primitive" entry; other entries of the file stay).

    python tools/inflate_bench.py [--reads 50000] [--runs 3] [--threads 16] [--out profiles/gpu_inflate.json]

--stream: the same for PLAIN gzip — the FASTQ compressed as `gzip -1` writes it, one member — through Engine.gunzip_stream
(DESIGN 7q): the five steps by device events and the whole call, against host.text_from_file on the same file (one thread's
work for such a file, whatever --threads says).  --chunk sets the decoder's chunk (0: the default).  Writes the "primitive"
entry of profiles/gpu_gunzip_stream.json.
"""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import yacrd_amd  # noqa: E402
from yacrd_amd import host  # noqa: E402


def stream(a):
    d = os.environ.get("YACRD_EDIT_BENCH_DIR", "/dev/shm")
    tag = os.path.join(d, "yacrd_ifs_%d_" % os.getpid())
    fq, gz = tag + "s.fastq", tag + "s.fastq.gz"
    out = a.out if os.path.basename(a.out) != "gpu_inflate.json" else os.path.join(ROOT, "profiles", "gpu_gunzip_stream.json")
    try:
        host.synth_fastq(host.SYNTH_SEQUEL, a.reads, a.overlaps, 20241108 + 5, a.reads // 200, fq)
        text = open(fq, "rb").read()
        os.remove(fq)
        c = zlib.compressobj(1, zlib.DEFLATED, 31)
        with open(gz, "wb") as f:
            for i in range(0, len(text), 1 << 26):
                f.write(c.compress(text[i:i + (1 << 26)]))
            f.write(c.flush())
        blob = open(gz, "rb").read()
        row = {"text_bytes": len(text), "gz_bytes": len(blob), "level": 1, "chunk": a.chunk, "runs": a.runs, "host_threads": a.threads,
               "device": [], "host": []}
        with yacrd_amd.Engine(device_id=0) as e:
            e.debug_gunzip_chunk(a.chunk)
            for k in range(a.runs + 1):  # (the first: buffers, code objects, the pinned arena)
                t0 = time.perf_counter()
                got = e.gunzip_stream(blob)
                call = time.perf_counter() - t0
                assert got == text, "the device's text differs"
                del got
                if k:
                    row["device"].append(dict(e.gunzip_stream_stats, call_ms=round(call * 1e3, 2)))
        for k in range(a.runs + 1):
            t0 = time.perf_counter()
            t = host.text_from_file(gz, a.threads)
            call = time.perf_counter() - t0
            assert t is not None and t.bytes() == text, "the host's text differs"
            t.close()
            if k:
                row["host"].append({"call_ms": round(call * 1e3, 2)})
        steps = ("find_ms", "size_ms", "symbols_ms", "windows_ms", "bytes_ms")
        row["device_steps_ms_slowest"] = max(sum(r[s] for s in steps) for r in row["device"])
        row["windows_us_per_span_slowest"] = max(1e3 * r["windows_ms"] / max(1, r["n_spans"]) for r in row["device"])
        row["device_call_ms_slowest"] = max(r["call_ms"] for r in row["device"])
        row["host_call_ms_fastest"] = min(r["call_ms"] for r in row["host"])
        print(json.dumps(row), flush=True)
        res = {}
        if os.path.exists(out):
            with open(out) as f:
                res = json.load(f)
        res["primitive" if not a.chunk else "primitive_chunk_%d" % a.chunk] = row
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    finally:
        for x in (fq, gz):
            if os.path.exists(x):
                os.remove(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--reads", type=int, default=50_000)
    ap.add_argument("--overlaps", type=int, default=5_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_inflate.json"))
    a = ap.parse_args()
    if a.stream:
        return stream(a)
    d = os.environ.get("YACRD_EDIT_BENCH_DIR", "/dev/shm")
    tag = os.path.join(d, "yacrd_ifb_%d_" % os.getpid())
    fq, gz = tag + "s.fastq", tag + "s.fastq.gz"
    try:
        host.synth_fastq(host.SYNTH_SEQUEL, a.reads, a.overlaps, 20241108 + 5, a.reads // 200, fq)
        text = open(fq, "rb").read()
        os.remove(fq)
        with yacrd_amd.Engine(device_id=0) as e:
            with e.gzip_writer(gz) as w:
                for i in range(0, len(text), 1 << 26):
                    w.write(text[i:i + (1 << 26)])
            blob = open(gz, "rb").read()
            row = {"text_bytes": len(text), "bgzf_bytes": len(blob), "runs": a.runs, "host_threads": a.threads, "device": [], "host": []}
            for k in range(a.runs + 1):  # (the first: buffers, code objects, the pinned arena)
                t0 = time.perf_counter()
                got = e.gunzip(blob)
                call = time.perf_counter() - t0
                assert got == text, "the device's text differs"
                del got
                if k:
                    row["device"].append(dict(e.gunzip_stats, call_ms=round(call * 1e3, 2)))
            for k in range(a.runs + 1):
                t0 = time.perf_counter()
                t = host.text_from_file(gz, a.threads)
                call = time.perf_counter() - t0
                assert t is not None and t.bytes() == text, "the host's text differs"
                threads, members = t.threads, t.members
                t.close()
                if k:
                    row["host"].append({"call_ms": round(call * 1e3, 2), "threads": threads, "members": members})
        row["kernel_ms_slowest"] = max(r["kernel_ms"] for r in row["device"])
        row["device_parts_ms_slowest"] = max(r["walk_ms"] + r["h2d_ms"] + r["kernel_ms"] + r["d2h_ms"] for r in row["device"])  # (without Python's copy)
        row["device_call_ms_slowest"] = max(r["call_ms"] for r in row["device"])
        row["host_call_ms_fastest"] = min(r["call_ms"] for r in row["host"])
        print(json.dumps(row), flush=True)
        res = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        res["primitive"] = row
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    finally:
        for x in (fq, gz):
            if os.path.exists(x):
                os.remove(x)


if __name__ == "__main__":
    main()
