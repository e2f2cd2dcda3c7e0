#!/usr/bin/env python3
"""tools/edit_fastq_bench.py --parent-bin PATH [--parent-again] [--fasta] [--window BYTES] [--reads R] [--overlaps O] [--runs K] [--ops scrubb,filter] [--forms plain,gzip1,bgzf] [--json PATH]
scrubb / filter on a FASTQ through the COMMAND, the parent commit's `yacrd` against this tree's, on a synthetic Sequel FASTQ
(50 000 reads: about 1 GB) in /dev/shm, output there too:
    yacrd -i s.paf -o r.yacrd -c 3 -n 0.4 <op> -i reads.fastq[.gz] -o out.fastq[.gz]
with the FASTQ plain, as gzip level 1 (one stream) and as BGZF; K timed runs of each binary after one warm-up, the old output
removed before the clock starts:
  (a) parent   PATH: the host editors — chunk-parallel on the plain file; for gzip one thread inflates and edits and the
               bytes leave through the gzip writer (its "[info] device deflate:" line)
  (b) new      this tree's yacrd: the text in HBM, cut, decided and gathered there (its "[info] device fastq editor:" line);
               for gzip the file inflated member-parallel and the output deflated where it lies
               for BGZF the file goes up compressed and is inflated on the device (its "[info] device inflate:" line;
               YACRD_NO_DEVICE_INFLATE=1 in the environment gives the rows of the host inflate instead)
The figures compared are the `edit` stage of YACRD_CLI_TIMING — slowest (b) against fastest (a) — and the wall clock.  Every
output is compared with the parent's (gzip: the inflated bytes when the streams differ).  One JSON line per op and form,
appended to --json (default profiles/edit_fastq.json).
--fasta: the same reads as FASTA, 80 bases a line (reads.fasta[.gz]): the device path is yacrd_engine_edit_fasta, its line
"[info] device fasta editor:", the default --json profiles/edit_fasta.json.
--window BYTES: the editor's windows (with --fasta 7l) against its whole-text run, in the same call: the "new" series runs
with YACRD_SEQ_WINDOW=18446744073709551615 (never windows), a third series "windowed" with YACRD_SEQ_WINDOW=BYTES; its output
is compared with the parent's too, and the row says whether the windowed run's slowest `edit` is ahead of the whole-text
run's fastest (the rule for the default).  The default --json is then profiles/edit_fastq_windows.json, with --fasta
profiles/edit_fasta_windows.json.
--window BYTES --forms bgzf: the BGZF-in form in windows, FASTQ or --fasta: the windows are cut where members end,
every window's members inflated on the device.  Both new series must show the "[info] device inflate:" line — a run that fell
back to the host inflate would report windows too, the gzip form's — and the default --json is profiles/edit_bgzf_windows.json
for both formats (the rows say which: "kind").
--parent-again: a second series of the parent behind the new one ("parent_again" in the row): what drifted meanwhile shows.
Where the parent has a device editor too, the figure to compare is the `kernels ... ms` of the info lines, not the stage."""
import argparse, gzip, json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yacrd_amd  # noqa: E402
from yacrd_amd import host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=50_000)
ap.add_argument("--overlaps", type=int, default=5_000_000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--ops", default="scrubb,filter")
ap.add_argument("--forms", default="plain,gzip1,bgzf")
ap.add_argument("--parent-bin", default=None)
ap.add_argument("--fasta", action="store_true")
ap.add_argument("--parent-again", action="store_true")
ap.add_argument("--window", type=int, default=0)
ap.add_argument("--json", default=None)
a = ap.parse_args()
kind = "fasta" if a.fasta else "fastq"
a.json = a.json or os.path.join(ROOT, "profiles", "edit_%s%s.json" % ("bgzf" if a.window and a.forms == "bgzf" else kind, "_windows" if a.window else ""))
editor_line = "[info] device %s editor:" % kind
if not a.parent_bin or not os.access(a.parent_bin, os.X_OK):
    sys.exit("--parent-bin: the yacrd binary built from the parent commit")
new_bin = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
d = os.environ.get("YACRD_EDIT_BENCH_DIR", "/dev/shm")
tag = os.path.join(d, "yacrd_efb_%d_" % os.getpid())
paf, fq, rep = tag + "s.paf", tag + "s.fastq", tag + "r.yacrd"


def to_fasta(src, dst):
    """the FASTQ's records as FASTA, 80 bases a line"""
    with open(src, "rb") as f, open(dst, "wb") as g:
        while True:
            head, seq = f.readline(), f.readline().rstrip(b"\n")
            if not head:
                return
            f.readline(), f.readline()
            g.write(b">" + head[1:] + b"".join(seq[i:i + 80] + b"\n" for i in range(0, len(seq), 80)))


def fresh(path):
    if os.path.exists(path):
        os.remove(path)  # (or the open's truncation frees the last run's pages inside the timed region)


def same(x, y, inflate):
    def chunks(p):
        with (gzip.open(p, "rb") if inflate else open(p, "rb")) as f:
            while True:
                b = f.read(1 << 24)
                yield b
                if not b:
                    return
    return all(p == q for p, q in zip(chunks(x), chunks(y)))


def run(binary, op, src, out, **env):
    rows = []
    for k in range(a.runs + 1):
        fresh(out)
        fresh(rep)
        t0 = time.perf_counter()
        p = subprocess.run([binary, "-i", paf, "-o", rep, "-c", "3", "-n", "0.4", op, "-i", src, "-o", out],
                           capture_output=True, text=True, env=dict(os.environ, YACRD_CLI_TIMING="1", **env))
        wall = time.perf_counter() - t0
        assert p.returncode == 0, p.stderr
        stages = dict(re.findall(r"^\[timing\] (\S+) ([0-9.]+) s$", p.stderr, re.M))
        info = [l for l in p.stderr.splitlines() if l.startswith(editor_line) or l.startswith("[info] device deflate:") or l.startswith("[info] device inflate:") or l.startswith("[info] device gunzip:")]
        row = {"edit_s": float(stages["edit"]), "wall_s": round(wall, 3), "info": info}
        if k:
            rows.append(row)
    return rows


made = [paf, fq, rep]
try:
    seed = 20241108 + 5
    host.synth_paf(host.SYNTH_SEQUEL, a.reads, a.overlaps, seed, paf)
    host.synth_fastq(host.SYNTH_SEQUEL, a.reads, a.overlaps, seed, a.reads // 200, fq)
    if a.fasta:
        to_fasta(fq, tag + "s.fasta")
        fresh(fq)
        fq = tag + "s.fasta"
        made.append(fq)
    size = os.path.getsize(fq)
    for form in a.forms.split(","):
        ext = "." + kind if form == "plain" else "." + kind + ".gz"
        src = fq if form == "plain" else tag + form + ext
        if form == "gzip1":
            with open(src, "wb") as f:
                subprocess.check_call(["gzip", "-1", "-c", fq], stdout=f)
        elif form == "bgzf":
            with yacrd_amd.Engine(device_id=0) as e, e.gzip_writer(src) as w, open(fq, "rb") as f:
                while True:
                    piece = f.read(1 << 26)
                    if not piece:
                        break
                    w.write(piece)
        made.append(src)
        for op in a.ops.split(","):
            old, new = tag + "old" + ext, tag + "new" + ext
            made.extend([old, new])
            parent = run(a.parent_bin, op, src, old)
            mine = run(new_bin, op, src, new, **({"YACRD_SEQ_WINDOW": str(2 ** 64 - 1)} if a.window else {}))
            windowed = None
            if a.window:
                assert same(old, new, False) or (form != "plain" and same(old, new, True)), "the whole-text run's output differs from the parent's"
                windowed = run(new_bin, op, src, new, YACRD_SEQ_WINDOW=str(a.window))
                assert all(int(l.rsplit("windows=", 1)[1]) > 1 for r in windowed for l in r["info"] if l.startswith(editor_line)), "not in windows"
                if form == "bgzf":  # (the windows of the device inflate, not the gzip form's behind a host inflate)
                    assert all(any(l.startswith("[info] device inflate:") for l in r["info"]) for r in mine + windowed), "the device inflate did not run"
            again = run(a.parent_bin, op, src, old) if a.parent_again else None
            assert any(l.startswith(editor_line) for l in mine[-1]["info"]), "the device editor did not run"
            assert same(old, new, False) or (form != "plain" and same(old, new, True)), "the new path's output differs from the parent's"
            worst_new, best_old = max(r["edit_s"] for r in mine), min(r["edit_s"] for r in parent)
            row = {"kind": kind, "reads": a.reads, "overlaps": a.overlaps, "op": op, "form": form, "text_bytes": size, "in_bytes": os.path.getsize(src),
                   "out_bytes": os.path.getsize(new), "parent": parent, "new": mine, "edit_stage_slowest_new_s": worst_new,
                   "edit_stage_fastest_parent_s": best_old, "ratio": round(best_old / worst_new, 2),
                   "wall_slowest_new_s": max(r["wall_s"] for r in mine), "wall_fastest_parent_s": min(r["wall_s"] for r in parent)}
            if windowed:
                worst_w, best_whole = max(r["edit_s"] for r in windowed), min(r["edit_s"] for r in mine)
                row.update({"window_bytes": a.window, "windowed": windowed, "edit_stage_slowest_windowed_s": worst_w,
                            "edit_stage_fastest_whole_s": best_whole, "windowed_ahead": worst_w < best_whole,
                            "ratio_windowed": round(best_old / worst_w, 2), "wall_slowest_windowed_s": max(r["wall_s"] for r in windowed)})
            if again:
                row["parent_again"] = again
            line = json.dumps(row)
            print(line, flush=True)
            with open(a.json, "a") as f:
                f.write(line + "\n")
            fresh(old)
            fresh(new)
        if src != fq:
            fresh(src)
finally:
    for x in made:
        fresh(x)
