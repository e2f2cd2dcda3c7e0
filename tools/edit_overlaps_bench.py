#!/usr/bin/env python3
"""tools/edit_overlaps_bench.py [--parent-again] [--reads R] [--overlaps O] [--runs K] [--op filter|extract] [--json PATH]
filter / extract on an OVERLAP file, host loop against device editor, on a synthetic PAF in /dev/shm (output there too);
K timed runs of each after one warm-up:
  (a) host     yacrd_edit_file: the one-thread loop (seconds, GB/s of input)
  (b) moved    yacrd_engine_edit_overlaps, the text moved to HBM (warm buffers), with text_ms / kernel_ms / out_ms
  (c) reused   the same from the mirror the device parser left in HBM
  (d) floor    yacrd_ingest_stats.text_ms of the device parser on the file: what moving the text in costs by itself
Every output is compared with the host loop's.  One JSON line (appended to --json when given).

--gzip --parent-bin PATH [--forms gzip1,bgzf]: the COMMAND on a gzip overlap file,
    yacrd -i ovl.paf.gz -o r.yacrd -c 3 -n 0.4 <op> -i ovl.paf.gz -o kept.paf.gz
with the same synthetic PAF as gzip level 1 (one stream) and as BGZF, K timed runs after one warm-up of
  (a) parent   PATH: the `yacrd` of the parent commit — the file inflated a second time, the host loop, the edited bytes through
               the gzip writer (its "[info] device deflate:" line)
  (b) new      this tree's yacrd — the detection's text reused, edited and deflated in HBM (its "[info] device editor + deflate:" line, on stdout)
and the `edit` stage of YACRD_CLI_TIMING as the figure compared: slowest (b) against fastest (a).  Every output is compared
with the parent's, byte for byte.  One JSON line per form (appended to --json when given).
--bgzf-in [--parent-bin PATH]: the same command on the synthetic PAF as BGZF, for the detection's own file and for a copy of it
(another inode), K timed runs after one warm-up of
  (a) host inflate    PATH, or without it this tree's yacrd with YACRD_NO_DEVICE_INFLATE=1 (the parent's route, unchanged)
  (b) device inflate  this tree's yacrd with YACRD_DEVICE_INFLATE=1: the file ingested compressed and edited where the ingest left
                      it (resident=1), or — the copy — inflated in HBM by the editor's own _bgzf_ form
with the stages inflate + detect + edit of YACRD_CLI_TIMING as the figure compared (slowest (b) against fastest (a)), the
editor's and the decoder's own stats per run, every output compared byte for byte (-c 4 -n 0.4 here).  One JSON line per case, and one
more for the same calls warm in ONE process: Engine.ingest_bgzf + edit_overlaps_resident, and edit_overlaps_bgzf, K runs after a warm-up.
--parent-again: a second series of the parent behind the new one ("parent_again" in the row): what drifted meanwhile shows.
  (--window without --bgzf-in, where the routes take turns: the parent once more at the end of every turn)
--window BYTES --parent-bin PATH [--gzip]: the overlap editor in windows against the whole-text run.  The command
    yacrd -i r.yacrd -o r2.yacrd -t 0 <op> -i ovl.paf -o kept.paf
(the detection read from a report: the text is moved, no mirror serves) on the synthetic PAF — with --gzip on its gzip -1 form, which
the command inflates on the host, edits as text and deflates on the device —, K timed rounds after one warm-up, every round running
  (i)   parent    PATH: the `yacrd` of the parent commit, the whole text at once
  (ii)  whole     this tree's yacrd with YACRD_EDIT_WINDOW=18446744073709551615: never windows
  (iii) windows   this tree's yacrd with YACRD_EDIT_WINDOW=BYTES
one behind the other, so that what drifts meanwhile touches all three alike.  Per run the `edit` stage and the wall time, the
stages of the editor's info line and its windows; then, in this process, what the device held for (ii) and (iii) and the ring's
bytes (Engine.edit_windows).  Every output is compared with the parent's byte for byte.  The two conditions of DESIGN 7n are
worked out in the row: whether (ii)'s kernel_ms and wall time lie within the spread of (i)'s runs, and whether the slowest (iii)
is under the fastest whole-text run.  One JSON line (appended to --json when given).
--bgzf-in --window BYTES --parent-bin PATH [--resident]: the same three columns on the synthetic PAF as BGZF.  Without
--resident the command is the one above on the BGZF file — the editor's own _bgzf_ form inflates it in HBM, window by window in
(iii); with it the detection reads the BGZF file itself (YACRD_DEVICE_INFLATE=1: ingested compressed) and the edit runs on the text
the ingest left in HBM, in windows from that mirror in (iii).  Per run also the decoder's kernel time; `held` as above."""
import argparse, json, os, re, subprocess, sys, time
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
ap.add_argument("--gzip", action="store_true")
ap.add_argument("--bgzf-in", action="store_true")
ap.add_argument("--parent-bin", default=None)
ap.add_argument("--parent-again", action="store_true")
ap.add_argument("--forms", default="gzip1,bgzf")
ap.add_argument("--window", type=int, default=0)
ap.add_argument("--resident", action="store_true")
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


def gzip_bench():
    new_bin = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
    if not a.parent_bin or not os.access(a.parent_bin, os.X_OK):
        sys.exit("--gzip needs --parent-bin: the yacrd binary built from the parent commit")
    made = [paf]
    try:
        host.synth_paf(host.SYNTH_SEQUEL, a.reads, a.overlaps, 20241108 + 5, paf)
        size = os.path.getsize(paf)
        for form in a.forms.split(","):
            src, rep, old, new = tag + form + ".paf.gz", tag + "r.yacrd", tag + "old.paf.gz", tag + "new.paf.gz"
            made.extend([src, rep, old, new])
            t0 = time.perf_counter()
            if form == "gzip1":
                with open(src, "wb") as f:
                    subprocess.check_call(["gzip", "-1", "-c", paf], stdout=f)
            else:
                with yacrd_amd.Engine(device_id=0) as e, e.gzip_writer(src) as w, open(paf, "rb") as f:
                    while True:
                        piece = f.read(1 << 26)
                        if not piece:
                            break
                        w.write(piece)
            made_s = time.perf_counter() - t0

            def run(binary, out):
                rows = []
                for k in range(a.runs + 1):
                    fresh(out)
                    fresh(rep)
                    t0 = time.perf_counter()
                    p = subprocess.run([binary, "-i", src, "-o", rep, "-t", "0", "-c", "3", "-n", "0.4", a.op, "-i", src, "-o", out],
                                       capture_output=True, text=True, env=dict(os.environ, YACRD_CLI_TIMING="1"))
                    wall = time.perf_counter() - t0
                    assert p.returncode == 0, p.stderr
                    stages = dict(re.findall(r"^\[timing\] (\S+) ([0-9.]+) s$", p.stderr, re.M))
                    info = [l for l in (p.stdout + p.stderr).splitlines() if l.startswith("[info] device editor + deflate:") or l.startswith("[info] device deflate:")]
                    assert len(info) == 1, p.stderr
                    row = {"edit_s": float(stages["edit"]), "inflate_s": float(stages.get("inflate", 0.0)), "detect_s": float(stages["detect"]), "wall_s": round(wall, 3)}
                    for name, key in (("inflate", "edit_inflate_ms"), ("text", "text_ms"), ("table", "table_ms"), ("editor kernels", "editor_kernel_ms"),
                                      ("encoder kernels", "encoder_kernel_ms"), ("kernels", "encoder_kernel_ms"), ("out", "out_ms"), ("h2d", "h2d_ms"),
                                      ("d2h", "d2h_ms"), ("write", "write_ms")):
                        m = re.search(r"(?:, |: )%s ([0-9.]+) ms" % name, info[0])
                        if m and key not in row:
                            row[key] = float(m.group(1))
                    m = re.search(r"text_reused=(\d)", info[0])
                    if m:
                        row["text_reused"] = int(m.group(1))
                    if k:
                        rows.append(row)
                return rows
            parent = run(a.parent_bin, old)
            mine = run(new_bin, new)
            if a.parent_again:
                again = run(a.parent_bin, old)
            assert same(old, new), "the new path's file differs from the parent's"
            worst_new, best_old = max(r["edit_s"] for r in mine), min(r["edit_s"] for r in parent)
            row = {"reads": a.reads, "overlaps": a.overlaps, "op": a.op, "form": form, "text_bytes": size, "gz_in_bytes": os.path.getsize(src),
                   "gz_out_bytes": os.path.getsize(new), "make_input_s": round(made_s, 2), "parent": parent, "new": mine,
                   "edit_stage_slowest_new_s": worst_new, "edit_stage_fastest_parent_s": best_old, "ratio": round(best_old / worst_new, 2)}
            if a.parent_again:
                row["parent_again"] = again
            line = json.dumps(row)
            print(line, flush=True)
            if a.json:
                with open(a.json, "a") as f:
                    f.write(line + "\n")
            for x in (src, old, new):
                fresh(x)
    finally:
        for x in made:
            fresh(x)


def bgzf_in_bench():
    """--bgzf-in: the command on a BGZF overlap file with the device inflate (YACRD_DEVICE_INFLATE=1: ingested compressed and
    edited where the ingest left it; for another BGZF file, the editor's own _bgzf_ form) against the host inflate"""
    new_bin = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
    old_bin = a.parent_bin or new_bin  # (without the parent's binary: this tree's with the device inflate switched off, the parent's route)
    if a.parent_bin and not os.access(a.parent_bin, os.X_OK):
        sys.exit("--parent-bin: not an executable")
    src, cp, rep, old, new = tag + "in.paf.gz", tag + "copy.paf.gz", tag + "r.yacrd", tag + "old.paf.gz", tag + "new.paf.gz"
    made = [paf, src, cp, rep, old, new]
    try:
        host.synth_paf(host.SYNTH_SEQUEL, a.reads, a.overlaps, 20241108 + 5, paf)
        size = os.path.getsize(paf)
        with yacrd_amd.Engine(device_id=0) as e, e.gzip_writer(src) as w, open(paf, "rb") as f:
            while True:
                piece = f.read(1 << 26)
                if not piece:
                    break
                w.write(piece)
        with open(src, "rb") as f, open(cp, "wb") as g:
            g.write(f.read())
        fresh(paf)

        def run(binary, sub_in, out, **env):
            rows = []
            base = {k: v for k, v in os.environ.items() if k not in ("YACRD_DEVICE_INFLATE", "YACRD_NO_DEVICE_INFLATE")}
            for k in range(a.runs + 1):
                fresh(out)
                fresh(rep)
                t0 = time.perf_counter()
                p = subprocess.run([binary, "-i", src, "-o", rep, "-t", "0", "-c", "4", "-n", "0.4", a.op, "-i", sub_in, "-o", out],
                                   capture_output=True, text=True, env=dict(base, YACRD_CLI_TIMING="1", **env))
                wall = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr
                stages = {k2: float(v) for k2, v in re.findall(r"^\[timing\] (\S+) ([0-9.]+) s$", p.stderr, re.M)}
                info = [l for l in p.stdout.splitlines() if l.startswith("[info] device editor + deflate:")]
                assert len(info) == 1, p.stdout + p.stderr
                row = {"ingest_to_edit_s": round(stages.get("inflate", 0.0) + stages["detect"] + stages["edit"], 4), "wall_s": round(wall, 3),
                       "inflate_s": stages.get("inflate", 0.0), "detect_s": stages["detect"], "edit_s": stages["edit"]}
                for name, key in (("inflate", "edit_inflate_ms"), ("text", "text_ms"), ("table", "table_ms"), ("editor kernels", "editor_kernel_ms"),
                                  ("encoder kernels", "encoder_kernel_ms"), ("out", "out_ms")):
                    m = re.search(r", %s ([0-9.]+) ms" % name, info[0])
                    if m:
                        row[key] = float(m.group(1))
                for flag in ("text_reused", "resident", "device_inflate"):
                    m = re.search(r"%s=(\d)" % flag, info[0])
                    if m:
                        row[flag] = int(m.group(1))
                for l in p.stderr.splitlines():
                    m = re.match(r"\[info\] device inflate: .* walk ([0-9.]+) ms, h2d ([0-9.]+) ms, kernels ([0-9.]+) ms", l)
                    if m:
                        row["inflate_walk_ms"], row["inflate_h2d_ms"], row["inflate_kernel_ms"] = (float(x) for x in m.groups())
                if k:
                    rows.append(row)
            return rows

        for case, sub_in in (("same file", src), ("another file", cp)):
            parent = run(old_bin, sub_in, old, **({} if a.parent_bin else {"YACRD_NO_DEVICE_INFLATE": "1"}))
            mine = run(new_bin, sub_in, new, YACRD_DEVICE_INFLATE="1")
            assert all(r.get("device_inflate") == 1 for r in mine), mine
            assert same(old, new), "the new route's file differs from the other's"
            worst_new, best_old = max(r["ingest_to_edit_s"] for r in mine), min(r["ingest_to_edit_s"] for r in parent)
            row = {"reads": a.reads, "overlaps": a.overlaps, "op": a.op, "case": case, "text_bytes": size, "bgzf_in_bytes": os.path.getsize(src),
                   "gz_out_bytes": os.path.getsize(new), "other": "parent binary" if a.parent_bin else "this binary, YACRD_NO_DEVICE_INFLATE=1",
                   "host_inflate": parent, "device_inflate": mine, "slowest_device_inflate_s": worst_new, "fastest_host_inflate_s": best_old,
                   "device_inflate_is_default_by_the_rule": worst_new < best_old}
            line = json.dumps(row)
            print(line, flush=True)
            if a.json:
                with open(a.json, "a") as f:
                    f.write(line + "\n")

        # warm, in one process: the calls the two routes are made of, K timed after one warm-up each, by their own stats
        import numpy as np
        blob = np.fromfile(src, dtype=np.uint8)
        warm = {"case": "warm in-process", "op": a.op, "text_bytes": size, "bgzf_in_bytes": int(blob.size), "ingest_bgzf": [], "edit_resident": [],
                "edit_bgzf": []}
        rnd = lambda d: {k2: (round(v, 2) if isinstance(v, float) else v) for k2, v in d.items()}  # noqa: E731
        with yacrd_amd.Engine(device_id=0) as e:
            for k in range(a.runs + 1):
                t0 = time.perf_counter()
                res, names, lengths, st = e.ingest_bgzf((blob.ctypes.data, int(blob.size)), 4, 0.4)
                t1 = time.perf_counter()
                fresh(new)
                es, gs = e.edit_overlaps_resident(op, names, res.read_type, out_path=new)
                t2 = time.perf_counter()
                assert es["mirror_reused"] == 1 and same(old, new)
                if k:
                    inf = st.pop("inflate")
                    warm["ingest_bgzf"].append({"s": round(t1 - t0, 4), **rnd(st), "inflate": rnd(inf)})
                    warm["edit_resident"].append({"s": round(t2 - t1, 4), "edit": rnd(es), "gzip": rnd(gs)})
            for k in range(a.runs + 1):
                fresh(new)
                t0 = time.perf_counter()
                es, gs = e.edit_overlaps_bgzf(op, blob, names, res.read_type, 1, out_path=new)
                dt = time.perf_counter() - t0
                assert same(old, new)
                if k:
                    warm["edit_bgzf"].append({"s": round(dt, 4), "edit": rnd(es), "gzip": rnd(gs), "inflate": rnd(e.inflate_stats)})
            e.trim()
        line = json.dumps(warm)
        print(line, flush=True)
        if a.json:
            with open(a.json, "a") as f:
                f.write(line + "\n")
    finally:
        for x in made:
            fresh(x)


def bgzf_window_bench():
    """--bgzf-in --window [--resident]: the command's edit of a BGZF overlap file: parent, this tree whole, this tree in windows"""
    import numpy as np
    new_bin = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
    if not a.parent_bin or not os.access(a.parent_bin, os.X_OK):
        sys.exit("--window needs --parent-bin: the yacrd binary built from the parent commit")
    src, rep, rep2 = tag + "in.paf.gz", tag + "r.yacrd", tag + "r2.yacrd"
    outs = {"parent": tag + "old.paf.gz", "whole": tag + "whole.paf.gz", "windows": tag + "win.paf.gz"}
    made = [paf, src, rep, rep2] + list(outs.values())
    never = str(2 ** 64 - 1)
    routes = (("parent", a.parent_bin, {}), ("whole", new_bin, {"YACRD_EDIT_WINDOW": never}), ("windows", new_bin, {"YACRD_EDIT_WINDOW": str(a.window)}))
    base = {k: v for k, v in os.environ.items() if k not in ("YACRD_EDIT_WINDOW", "YACRD_DEVICE_INFLATE", "YACRD_NO_DEVICE_INFLATE")}
    more = {"YACRD_DEVICE_INFLATE": "1"} if a.resident else {}
    try:
        host.synth_paf(host.SYNTH_SEQUEL, a.reads, a.overlaps, 20241108 + 5, paf)
        size = os.path.getsize(paf)
        p = subprocess.run([new_bin, "-i", paf, "-o", rep, "-t", "0", "-c", "3", "-n", "0.4"], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        with yacrd_amd.Engine(device_id=0) as e, e.gzip_writer(src) as w, open(paf, "rb") as f:
            while True:
                piece = f.read(1 << 26)
                if not piece:
                    break
                w.write(piece)
        fresh(paf)
        det = ["-i", src, "-o", rep2, "-t", "0", "-c", "3", "-n", "0.4"] if a.resident else ["-i", rep, "-o", rep2, "-t", "0"]
        rows = {name: [] for name, _, _ in routes}
        for k in range(a.runs + 1):
            for name, binary, env in routes:
                fresh(outs[name])
                fresh(rep2)
                t0 = time.perf_counter()
                p = subprocess.run([binary] + det + [a.op, "-i", src, "-o", outs[name]], capture_output=True, text=True,
                                   env=dict(base, YACRD_CLI_TIMING="1", **more, **env))
                wall = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr
                stages = dict(re.findall(r"^\[timing\] (\S+) ([0-9.]+) s$", p.stderr, re.M))
                info = [l for l in p.stdout.splitlines() if l.startswith("[info] device editor + deflate:")]
                assert len(info) == 1, p.stdout + p.stderr  # (the device editor ran: no fallback to the host inflate or the host loop)
                row = {"edit_s": float(stages["edit"]), "wall_s": round(wall, 3)}
                for label, key in (("text", "text_ms"), ("table", "table_ms"), ("editor kernels", "kernel_ms"), ("encoder kernels", "encoder_kernel_ms"), ("out", "out_ms")):
                    m = re.search(r", %s ([0-9.]+) ms" % label, info[0])
                    if m:
                        row[key] = float(m.group(1))
                for flag in ("resident", "device_inflate"):
                    row[flag] = int(re.search(r"%s=(\d)" % flag, info[0]).group(1))
                inf = [re.match(r"\[info\] device inflate: .* walk ([0-9.]+) ms, h2d ([0-9.]+) ms, kernels ([0-9.]+) ms", l) for l in p.stderr.splitlines()]
                inf = [m for m in inf if m]
                if inf:  # (the last one: the edit's, or — resident — the ingest's, the only one)
                    row["inflate_h2d_ms"], row["inflate_kernel_ms"] = float(inf[-1].group(2)), float(inf[-1].group(3))
                m = re.search(r" windows=(\d+)$", info[0])
                row["windows"] = int(m.group(1)) if m else 0  # (the parent's line does not say: it has none)
                if k:
                    rows[name].append(row)
        assert same(outs["parent"], outs["whole"]) and same(outs["parent"], outs["windows"]), "this tree's file differs from the parent's"
        assert all(r["resident"] == (1 if a.resident else 0) and r["device_inflate"] == 1 for rs in rows.values() for r in rs)
        assert all(r["windows"] == 0 for r in rows["whole"]) and all(r["windows"] > 1 for r in rows["windows"])
        # in this process: what the device holds behind the edit for the two routes of this tree
        held = {}
        blob = np.fromfile(src, dtype=np.uint8)
        with yacrd_amd.Engine(device_id=0) as e:
            res, names, lengths, _ = e.ingest_bgzf((blob.ctypes.data, int(blob.size)), 3, 0.4)
            for name, sw in (("whole", 2 ** 64 - 1), ("windows", a.window)):
                e.trim()  # (the parser's mirror goes with it)
                if a.resident:
                    e.ingest_bgzf((blob.ctypes.data, int(blob.size)), 3, 0.4)
                before = yacrd_amd.engine.live_bytes()[0]
                e.debug_edit_window(sw)
                fresh(got)
                if a.resident:
                    e.edit_overlaps_resident(op, names, res.read_type, out_path=got)
                else:
                    e.edit_overlaps_bgzf(op, blob, names, res.read_type, 1, out_path=got)
                held[name] = {"device_bytes_beside_what_was_held": int(yacrd_amd.engine.live_bytes()[0] - before), "live_bytes": int(yacrd_amd.engine.live_bytes()[0]),
                              **e.edit_windows()}
            e.trim()
        fresh(got)
        whole_like = rows["parent"] + rows["whole"]
        spread = lambda key: (min(r[key] for r in rows["parent"]), max(r[key] for r in rows["parent"]))  # noqa: E731
        row = {"reads": a.reads, "overlaps": a.overlaps, "op": a.op, "bgzf_in": True, "resident": bool(a.resident), "window": a.window, "text_bytes": size,
               "bgzf_in_bytes": os.path.getsize(src), "out_bytes": os.path.getsize(outs["parent"]), **rows, "held": held,
               "whole_kernel_ms_within_parent_spread": all(spread("kernel_ms")[0] <= r["kernel_ms"] <= spread("kernel_ms")[1] for r in rows["whole"]),
               "whole_edit_s_within_parent_spread": all(r["edit_s"] <= spread("edit_s")[1] for r in rows["whole"]),
               "whole_wall_s_within_parent_spread": all(r["wall_s"] <= spread("wall_s")[1] for r in rows["whole"]),
               "slowest_windows_edit_s": max(r["edit_s"] for r in rows["windows"]), "fastest_whole_edit_s": min(r["edit_s"] for r in whole_like),
               "windows_when_fits_by_the_rule": max(r["edit_s"] for r in rows["windows"]) < min(r["edit_s"] for r in whole_like)}
        line = json.dumps(row)
        print(line, flush=True)
        if a.json:
            with open(a.json, "a") as f:
                f.write(line + "\n")
    finally:
        for x in made + [got]:
            fresh(x)


def window_bench():
    """--window: the command's edit of a plain (or, --gzip, a gzip -1) overlap file: parent, this tree whole, this tree in windows"""
    import ctypes
    import numpy as np
    new_bin = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
    if not a.parent_bin or not os.access(a.parent_bin, os.X_OK):
        sys.exit("--window needs --parent-bin: the yacrd binary built from the parent commit")
    ext = ".paf.gz" if a.gzip else ".paf"
    src, rep, rep2 = (tag + "in.paf.gz" if a.gzip else paf), tag + "r.yacrd", tag + "r2.yacrd"
    outs = {"parent": tag + "old" + ext, "whole": tag + "whole" + ext, "windows": tag + "win" + ext}
    never = str(2 ** 64 - 1)
    routes = (("parent", a.parent_bin, {}), ("whole", new_bin, {"YACRD_EDIT_WINDOW": never}), ("windows", new_bin, {"YACRD_EDIT_WINDOW": str(a.window)}))
    if a.parent_again:  # (the parent once more in every turn, behind this tree's two: what drifts within a turn shows)
        routes += (("parent_again", a.parent_bin, {}),)
        outs["parent_again"] = tag + "old2" + ext
    made = [paf, src, rep, rep2] + list(outs.values())
    line_tag = "[info] device editor + deflate:" if a.gzip else "[info] device editor:"
    kernels = "editor kernels" if a.gzip else "kernels"
    base = {k: v for k, v in os.environ.items() if k != "YACRD_EDIT_WINDOW"}
    try:
        host.synth_paf(host.SYNTH_SEQUEL, a.reads, a.overlaps, 20241108 + 5, paf)
        size = os.path.getsize(paf)
        p = subprocess.run([new_bin, "-i", paf, "-o", rep, "-t", "0", "-c", "3", "-n", "0.4"], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        if a.gzip:
            with open(src, "wb") as f:
                subprocess.check_call(["gzip", "-1", "-c", paf], stdout=f)
        rows = {name: [] for name, _, _ in routes}
        for k in range(a.runs + 1):
            for name, binary, env in routes:
                fresh(outs[name])
                fresh(rep2)
                t0 = time.perf_counter()
                p = subprocess.run([binary, "-i", rep, "-o", rep2, "-t", "0", a.op, "-i", src, "-o", outs[name]], capture_output=True, text=True,
                                   env=dict(base, YACRD_CLI_TIMING="1", **env))
                wall = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr
                stages = dict(re.findall(r"^\[timing\] (\S+) ([0-9.]+) s$", p.stderr, re.M))
                info = [l for l in (p.stdout + p.stderr).splitlines() if l.startswith(line_tag)]
                assert len(info) == 1, p.stdout + p.stderr  # (the device editor ran: no fallback to the host loop)
                row = {"edit_s": float(stages["edit"]), "wall_s": round(wall, 3)}
                for label, key in (("text", "text_ms"), ("table", "table_ms"), (kernels, "kernel_ms"), ("encoder kernels", "encoder_kernel_ms"), ("out", "out_ms")):
                    m = re.search(r", %s ([0-9.]+) ms" % label, info[0])
                    if m:
                        row[key] = float(m.group(1))
                m = re.search(r" windows=(\d+)$", info[0])
                row["windows"] = int(m.group(1)) if m else 0  # (the parent's line does not say: it has none)
                if k:
                    rows[name].append(row)
        assert all(same(outs["parent"], outs[name]) for name in outs), "a file differs from the parent's first"
        assert all(r["windows"] == 0 for r in rows["whole"]) and all(r["windows"] == (size + a.window - 1) // a.window for r in rows["windows"])
        # in this process: what the device holds for the two routes of this tree (plain text out; with --gzip the members)
        held = {}
        if a.gzip:
            text = host.text_from_file(src)
        with yacrd_amd.Engine(device_id=0) as e:
            res, names, lengths, _ = e.ingest_paf(paf, 3, 0.4)
            for name, sw in (("whole", 2 ** 64 - 1), ("windows", a.window)):
                e.trim()  # (the parser's mirror goes with it: the text is moved)
                before = yacrd_amd.engine.live_bytes()[0]
                e.debug_edit_window(sw)
                fresh(got)
                if a.gzip:
                    buf = np.ctypeslib.as_array(ctypes.cast(text.address, ctypes.POINTER(ctypes.c_uint8)), shape=(text.n_bytes,))
                    e.edit_overlaps_gzip(op, buf, names, res.read_type, 1, out_path=got)
                else:
                    e.edit_overlaps(op, paf, got, names, res.read_type)
                held[name] = {"device_bytes": int(yacrd_amd.engine.live_bytes()[0] - before), **e.edit_windows()}
            e.trim()
        fresh(got)
        whole_like = rows["parent"] + rows["whole"]
        spread = lambda key: (min(r[key] for r in rows["parent"]), max(r[key] for r in rows["parent"]))  # noqa: E731
        row = {"reads": a.reads, "overlaps": a.overlaps, "op": a.op, "gzip": bool(a.gzip), "window": a.window, "text_bytes": size,
               "out_bytes": os.path.getsize(outs["parent"]), **rows, "held": held,
               "whole_kernel_ms_within_parent_spread": all(spread("kernel_ms")[0] <= r["kernel_ms"] <= spread("kernel_ms")[1] for r in rows["whole"]),
               "whole_wall_s_within_parent_spread": all(r["wall_s"] <= spread("wall_s")[1] for r in rows["whole"]),
               "slowest_windows_edit_s": max(r["edit_s"] for r in rows["windows"]), "fastest_whole_edit_s": min(r["edit_s"] for r in whole_like),
               "windows_when_fits_by_the_rule": max(r["edit_s"] for r in rows["windows"]) < min(r["edit_s"] for r in whole_like)}
        line = json.dumps(row)
        print(line, flush=True)
        if a.json:
            with open(a.json, "a") as f:
                f.write(line + "\n")
    finally:
        for x in made + [got]:
            fresh(x)


if a.window and a.bgzf_in:
    bgzf_window_bench()
    sys.exit(0)
if a.window:
    window_bench()
    sys.exit(0)
if a.bgzf_in:
    bgzf_in_bench()
    sys.exit(0)
if a.gzip:
    gzip_bench()
    sys.exit(0)

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
