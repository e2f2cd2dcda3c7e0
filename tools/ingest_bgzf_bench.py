#!/usr/bin/env python3
"""tools/ingest_bgzf_bench.py --parent-bin PATH [--runs K] [--inputs paf_bgzf,paf_gzip1,paf_plain,report_bgzf] [--report-reads R]
                               [--report-overlaps O] [--json PATH]
The detection through the COMMAND, the parent commit's `yacrd` against this tree's, inputs and reports in /dev/shm:
    yacrd -i <file> -o report.yacrd -c 4 -n 0.4
  paf_bgzf     BASELINE configs[1]'s PAF (100 k reads / 5 M overlaps, 367 MB) as BGZF from this project's encoder: the parent
               inflates on the host (its "[timing] inflate" stage), this tree sends the compressed bytes up and inflates them in
               HBM while they land (its "[info] device inflate:" line) — the row the CLI default is decided by
  paf_gzip1    the same PAF as `gzip -1`, one stream: both take the host inflate (recorded, not gated)
  paf_plain    the same PAF as text (recorded, not gated)
  report_bgzf  a 5 M-read report as BGZF, read back (-i report.yacrd.gz): decided like paf_bgzf
K timed runs of each binary after one warm-up.  `ingest_s` is what lies between engine_create and the report writer: the
stages `inflate` (where there is one) + `detect` of YACRD_CLI_TIMING.  The rule (DESIGN 7h's): the device route is the default
for a kind of input only when the SLOWEST new ingest_s is under the FASTEST parent ingest_s.  Every report written is compared
byte for byte with the parent's.
Then, in this process, one warm Engine.ingest_bgzf / ingest_report_bgzf of the BGZF files for the stages of one run (walk,
compressed bytes up, inflate kernels by device events, parse, build, run) — as built, segment-wise, and with
YACRD_BGZF_ONE_LAUNCH=1, which holds the decoder back until the whole stream has landed and launches it once.
One JSON object, written to --json (default profiles/ingest_bgzf.json)."""
import argparse, json, os, re, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yacrd_amd  # noqa: E402
from yacrd_amd import host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--inputs", default="paf_bgzf,paf_gzip1,paf_plain,report_bgzf")
ap.add_argument("--parent-bin", default=None)
ap.add_argument("--report-reads", type=int, default=5_000_000)
ap.add_argument("--report-overlaps", type=int, default=100_000_000)
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ingest_bgzf.json"))
a = ap.parse_args()
if not a.parent_bin or not os.access(a.parent_bin, os.X_OK):
    sys.exit("--parent-bin: the yacrd binary built from the parent commit")
new_bin = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
d = os.environ.get("YACRD_INGEST_BENCH_DIR", "/dev/shm")
tag = os.path.join(d, "yacrd_ibb_%d_" % os.getpid())
made = []


def fresh(path):
    if os.path.exists(path):
        os.remove(path)


def bgzf_file(src, dst):
    """src as BGZF from the device encoder"""
    with yacrd_amd.Engine(device_id=0) as e, e.gzip_writer(dst) as w, open(src, "rb") as f:
        while True:
            piece = f.read(1 << 26)
            if not piece:
                break
            w.write(piece)


def write_report(path):
    off, iv, lens = host.synth_csr(host.SYNTH_SEQUEL, a.report_reads, a.report_overlaps, 20241108 + 5)
    names = np.char.add("read_", np.arange(a.report_reads).astype(str)).astype("S").tolist()
    with yacrd_amd.Engine(device_id=0) as e:
        res = e.run(off, iv, lens, 3, 0.4)
        e.write_report(path, names, lens, res)


def run(binary, src, out):
    rows = []
    for k in range(a.runs + 1):
        fresh(out)
        t0 = time.perf_counter()
        p = subprocess.run([binary, "-i", src, "-o", out, "-c", "4", "-n", "0.4"], capture_output=True, text=True,
                           env=dict(os.environ, YACRD_CLI_TIMING="1", YACRD_DEVICE_INFLATE="1"))  # (the route under test, whatever the default)
        wall = time.perf_counter() - t0
        assert p.returncode == 0, p.stderr
        stages = {k2: float(v) for k2, v in re.findall(r"^\[timing\] (\S+) ([0-9.]+) s$", p.stderr, re.M)}
        info = [l for l in p.stderr.splitlines() if l.startswith("[info] device inflate:") or l.startswith("[info] device report reader:")]
        row = {"ingest_s": round(stages.get("inflate", 0.0) + stages["detect"], 4), "stages": stages, "wall_s": round(wall, 3), "info": info}
        if k:
            rows.append(row)
    return rows


def one_run(blob, report, one_launch):
    """the stages of one warm call in this process"""
    if one_launch:
        os.environ["YACRD_BGZF_ONE_LAUNCH"] = "1"
    try:
        with yacrd_amd.Engine(device_id=0) as e:
            call = (lambda: e.ingest_report_bgzf(blob, 0.4)) if report else (lambda: e.ingest_bgzf(blob, 4, 0.4))
            call()
            t0 = time.perf_counter()
            _, _, _, st = call()
            dt = time.perf_counter() - t0
    finally:
        os.environ.pop("YACRD_BGZF_ONE_LAUNCH", None)
    inf = st.pop("inflate")
    return {"call_ms": round(dt * 1e3, 2), "walk_ms": inf["walk_ms"], "h2d_ms": inf["h2d_ms"], "inflate_kernel_ms": inf["kernel_ms"],
            "n_members": inf["n_members"], "in_bytes": inf["in_bytes"], "out_bytes": inf["out_bytes"], "text_ms": st["text_ms"],
            "parse_ms": st["parse_ms"], "build_ms": st["build_ms"], "run_ms": st["run_ms"], "d2h_ms": st["d2h_ms"]}


out = {"tool": "ingest_bgzf_bench", "runs": a.runs, "command": "yacrd -i <file> -o report.yacrd -c 4 -n 0.4", "inputs": {}}
try:
    inputs = a.inputs.split(",")
    paf = tag + "s.paf"
    files = {}
    if any(i.startswith("paf") for i in inputs):
        host.synth_paf(host.SYNTH_ONT, 100_000, 5_000_000, 20241108 + 2, paf)
        made.append(paf)
        files["paf_plain"] = paf
        if "paf_bgzf" in inputs:
            files["paf_bgzf"] = tag + "bgzf.paf.gz"
            bgzf_file(paf, files["paf_bgzf"])
        if "paf_gzip1" in inputs:
            files["paf_gzip1"] = tag + "gzip1.paf.gz"
            with open(files["paf_gzip1"], "wb") as f:
                subprocess.check_call(["gzip", "-1", "-c", paf], stdout=f)
    if "report_bgzf" in inputs:
        rep = tag + "in.yacrd"
        write_report(rep)
        made.append(rep)
        files["report_bgzf"] = tag + "in.yacrd.gz"
        bgzf_file(rep, files["report_bgzf"])
        out["report_text_bytes"] = os.path.getsize(rep)
    made.extend(files.values())
    old, new = tag + "old.yacrd", tag + "new.yacrd"
    made.extend([old, new])
    for name in inputs:
        src = files[name]
        parent = run(a.parent_bin, src, old)
        mine = run(new_bin, src, new)
        with open(old, "rb") as f, open(new, "rb") as g:
            assert f.read() == g.read(), "%s: the report differs from the parent's" % name
        device = any(l.startswith("[info] device inflate:") for l in mine[-1]["info"])
        assert device == name.endswith("_bgzf"), "%s: the device inflate %s" % (name, "ran" if device else "did not run")
        worst_new, best_old = max(r["ingest_s"] for r in mine), min(r["ingest_s"] for r in parent)
        row = {"in_bytes": os.path.getsize(src), "report_bytes": os.path.getsize(new), "reports_equal": True, "device_inflate": device,
               "parent": parent, "new": mine, "ingest_slowest_new_s": worst_new, "ingest_fastest_parent_s": best_old,
               "ratio": round(best_old / worst_new, 2), "gated": name.endswith("_bgzf"),
               "wall_slowest_new_s": max(r["wall_s"] for r in mine), "wall_fastest_parent_s": min(r["wall_s"] for r in parent)}
        if row["gated"]:
            row["device_route_is_default"] = worst_new < best_old
            with open(src, "rb") as f:
                blob = f.read()
            row["one_run_segment_wise"] = one_run(blob, name.startswith("report"), False)
            row["one_run_one_launch_behind_the_upload"] = one_run(blob, name.startswith("report"), True)
            del blob
        out["inputs"][name] = row
        print(json.dumps({name: {k: v for k, v in row.items() if k not in ("parent", "new")}}), flush=True)
finally:
    for x in made:
        fresh(x)
with open(a.json, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
