#!/usr/bin/env python3
"""Device deflate: kernels alone (device events), the whole Engine.gzip call, size against zlib level 1 per block, and
the CLI's `edit` stage on a plain-gzip FASTQ with and without YACRD_NO_DEVICE_DEFLATE=1 (the latter is the path before
the device encoder).  Writes profiles/gpu_deflate.json.

    python tools/deflate_bench.py [--mb 1024] [--cli-mb 2048] [--repeats 5]
"""
import argparse
import gzip
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import yacrd_amd  # noqa: E402
from yacrd_amd import host  # noqa: E402
from deflate_cases import huffman_only_size, level1_size  # noqa: E402

BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def tile(data, n):
    return (data * (n // len(data) + 1))[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--cli-mb", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cli-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_deflate.json"))
    a = ap.parse_args()
    golden = os.path.join(ROOT, "tests", "golden")
    tmp = tempfile.mkdtemp(prefix="deflate_bench.")
    host.synth_fastq(host.SYNTH_ONT, 20000, 200000, 5, 100, os.path.join(tmp, "s.fastq"))
    host.synth_paf(host.SYNTH_ONT, 20000, 400000, 5, os.path.join(tmp, "s.paf"))
    corpora = {
        "golden_fastq_tiled": gzip.open(os.path.join(golden, "reads.fastq.gz"), "rb").read(),
        "synthetic_fastq": open(os.path.join(tmp, "s.fastq"), "rb").read(),
        "synthetic_paf": open(os.path.join(tmp, "s.paf"), "rb").read(),
    }
    res = {"mb": a.mb, "repeats": a.repeats, "corpora": {}}
    with yacrd_amd.Engine(device_id=0) as e:
        for name, base in corpora.items():
            sample = base[:32 << 20]
            blob = e.gzip(sample)
            row = {"sample_bytes": len(sample), "out": len(blob), "H": huffman_only_size(sample), "L": level1_size(sample)}
            row["out_over_L"], row["out_over_H"] = len(blob) / row["L"], len(blob) / row["H"]
            data = tile(base, a.mb << 20)
            e.gzip(data[:64 << 20])  # warm: buffers, code objects
            kern, call = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                out = e.gzip(data)
                call.append(len(data) / 1e9 / (time.perf_counter() - t0))
                kern.append(len(data) / 1e6 / e.gzip_stats["kernel_ms"])
            row.update(bytes=len(data), out_bytes=len(out), kernels_GBps=spread(kern), gzip_mem_GBps=spread(call),
                       n_stored=int(e.gzip_stats["n_stored"]))
            res["corpora"][name] = row
            print(name, json.dumps(row), flush=True)
            del data, out
    if a.cli_mb:
        # the CLI's edit stage on a plain-gzip FASTQ: device deflate against zlib's one thread
        paf = os.path.join(golden, "reads.paf")
        src = os.path.join(tmp, "reads.fastq.gz")
        text = tile(corpora["golden_fastq_tiled"], a.cli_mb << 20)
        text = text[:text.rfind(b"\n@") + 1]
        t0 = time.perf_counter()
        p = subprocess.Popen(["gzip", "-1", "-c"], stdin=subprocess.PIPE, stdout=open(src, "wb"))
        p.stdin.write(text)
        p.stdin.close()
        p.wait()
        cli = {"text_bytes": len(text), "gzip_1_seconds": time.perf_counter() - t0}
        del text
        for label, env in (("device_deflate", {}), ("zlib_one_thread", {"YACRD_NO_DEVICE_DEFLATE": "1"})):
            edits = []
            for _ in range(a.cli_repeats):
                r = subprocess.run([BIN, "-i", paf, "-o", os.path.join(tmp, "r.yacrd"), "scrubb", "-i", src, "-o", os.path.join(tmp, label + ".fastq.gz")],
                                   capture_output=True, text=True, env=dict(os.environ, YACRD_CLI_TIMING="1", **env))
                assert r.returncode == 0, r.stderr
                m = re.search(r"\[timing\] edit ([0-9.]+) s", r.stderr)
                edits.append(float(m.group(1)) if m else None)
                info = [l for l in r.stderr.splitlines() if "device deflate" in l]
            cli[label] = {"edit_seconds": edits, "edit_seconds_spread": spread(edits), "info": info, "out_bytes": os.path.getsize(os.path.join(tmp, label + ".fastq.gz")), "stderr_tail": r.stderr.splitlines()[-8:]}
        cli["speedup_median"] = cli["zlib_one_thread"]["edit_seconds_spread"]["median"] / cli["device_deflate"]["edit_seconds_spread"]["median"]
        cli["speedup_worst"] = cli["zlib_one_thread"]["edit_seconds_spread"]["min"] / cli["device_deflate"]["edit_seconds_spread"]["max"]
        res["cli_scrubb_plain_gzip_fastq"] = cli
        print(json.dumps(cli), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
