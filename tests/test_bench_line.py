"""bench.py's LAST stdout line is what the driver parses: compact (< 4 KB), strict JSON, the contract's keys with
`roofline` and `cpu_baseline` in it — everything else goes to bench_extras.json (a 30 KB line came
back `parsed: null`).  CPU check on the full object of a recorded run (profiles/r04_bench_default.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bad_const(name):
    raise ValueError(name)


def test_compact_line_from_a_recorded_full_object():
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_default.json")))
    full["headline"]["whole_path_frac_of_peak"] = float("nan")  # a NaN anywhere must not reach the line
    full["jitter"]["configs[1]"]["ms_per_step"] = float("inf")
    line = bench.compact_line(bench.no_nan(full), "/somewhere/bench_extras.json")
    s = json.dumps(line, allow_nan=False, separators=(",", ":"))
    assert len(s.encode()) < bench.COMPACT_LIMIT
    back = json.loads(s, parse_constant=_bad_const)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "parity", "roofline", "cpu_baseline"):
        assert k in back, k
    assert back["value"] == full["value"] and back["ms_per_step"] == full["ms_per_step"]
    assert "configs[4]" in back["config"]["workload"] and len(back["config"]["workload"]) <= 300
    r = back["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] == full["roofline"]["traffic"]
    assert back["cpu_baseline"]["cores"] == 16 and back["cpu_baseline"]["kind"] == "port"
    assert back["whole_path_frac_of_peak"] is None and back["jitter"]["configs[1]"][0] is None
    assert back["configs2_ms"] > 0 and back["skewed_ms"] > 0 and back["one_launch_us"] > 0
    assert back["extras"] == "bench_extras.json"


def test_compact_line_survives_failed_blocks():
    import bench
    full = {"metric": "reads_per_sec_classified", "value": 1.0, "unit": "reads/s", "n_gpus": 1, "steps": 1, "warmup": 1,
            "ms_per_step": 1.0, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u32",
            "data": "synthetic", "config": {"workload": "w" * 5000}, "parity": "bit-exact", "roofline": {"bound": "hbm"},
            "cpu_baseline": {"error": "x" * 100}, "configs2": {"error": "boom"}, "jitter": {"configs[1]": {"error": "e"}}}
    line = bench.compact_line(bench.no_nan(full), "not written: OSError()")
    s = json.dumps(line, allow_nan=False)
    assert len(s) < bench.COMPACT_LIMIT and line["configs2_ms"] is None and line["extras"].startswith("not written")


def test_gpus_flag_launches_the_ranks_itself(monkeypatch):
    """`--gpus N` was parsed and ignored.  Without a launcher and N > 1, bench.py becomes
    `python -m torch.distributed.run --nproc-per-node N ... bench.py <same arguments>`; N = 1 stays one process."""
    import argparse
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = {}

    def fake_execv(exe, cmd):
        seen["exe"], seen["cmd"] = exe, list(cmd)
        raise SystemExit(0)
    monkeypatch.setattr(bench.os, "execv", fake_execv)
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    try:
        bench.launch_ranks(argparse.Namespace(gpus=4))
    except SystemExit:
        pass
    cmd = seen["cmd"]
    assert seen["exe"] == sys.executable and cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "7"]
    seen.clear()
    for g in (None, 1):  # one rank: no launcher
        a = argparse.Namespace(gpus=g)
        bench.launch_ranks(a)
        assert a.gpus == 1 and not seen


def test_gpus_flag_must_agree_with_the_launcher(monkeypatch):
    import argparse
    import subprocess
    import bench
    monkeypatch.setenv("WORLD_SIZE", "2")
    a = argparse.Namespace(gpus=None)
    bench.launch_ranks(a)
    assert a.gpus == 2  # (no flag: the launcher's count)
    a = argparse.Namespace(gpus=2)
    bench.launch_ranks(a)
    assert a.gpus == 2
    # a disagreement stops the run before anything is loaded or measured
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert p.returncode == 2 and "WORLD_SIZE=2" in p.stderr and not p.stdout.strip()


def test_compact_line_limit_is_enforced_whatever_the_blocks_hold():
    """the line could still pass 4096 bytes once both optional blocks were dropped."""
    import bench
    full = {"metric": "reads_per_sec_classified", "value": 1.0, "unit": "reads/s", "n_gpus": 8, "steps": 1, "warmup": 1,
            "ms_per_step": 1.0, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u32",
            "data": "synthetic", "config": {"workload": "w" * 5000, "parallelism": "y" * 5000}, "parity": "p" * 5000,
            "roofline": {"bound": "hbm", "traffic_source_short": "z" * 3000}, "cpu_baseline": {"error": "x" * 5000},
            "headline": {"per_rank": [{"ms_per_step": 1.0}] * 8}}
    line = bench.compact_line(bench.no_nan(full), "e.json")
    s = json.dumps(line, allow_nan=False, separators=(",", ":"))
    assert len(s.encode()) < bench.COMPACT_LIMIT
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "parity", "roofline", "cpu_baseline"):
        assert k in line, k


def _fake_result(R, seed):
    import numpy as np
    from yacrd_amd.engine import Result
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 4, R)
    bo = np.concatenate(([0], np.cumsum(n))).astype(np.uint64)
    br = rng.integers(0, 60000, (int(bo[-1]), 2)).astype(np.uint32)
    return Result(bo, br, rng.integers(0, 3, R).astype(np.uint8))


def test_dump_outputs_is_a_fixed_sample_of_what_the_caller_receives(tmp_path, monkeypatch):
    """--dump-outputs: the engine's result on a fixed, seeded sample of the reads (all of them when few), as float32 /
    float64 .npy within the size limit, and the same files whether one rank or two held the reads."""
    import types
    import numpy as np
    import bench
    one = types.SimpleNamespace(dist=None, world=1, rank=0)
    got = _fake_result(5000, 1)

    def load(d):
        return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}

    bench.dump_outputs(one, got, 0, 5000, str(tmp_path / "all"))
    f = load(tmp_path / "all")
    assert set(f) == {"read_ids", "read_type", "bad_offsets", "bad_regions", "totals"}
    assert all(a.dtype in (np.float32, np.float64) for a in f.values())
    assert np.array_equal(f["read_ids"], np.arange(5000)) and np.array_equal(f["read_type"], got.read_type)
    assert np.array_equal(f["bad_offsets"], got.bad_offsets) and np.array_equal(f["bad_regions"], got.bad_regions)
    assert f["totals"].tolist() == [5000, int(got.bad_offsets[-1])] + np.bincount(got.read_type, minlength=3).tolist()

    monkeypatch.setattr(bench, "DUMP_READS", 700)  # more reads than the sample holds
    bench.dump_outputs(one, got, 0, 5000, str(tmp_path / "a"))
    bench.dump_outputs(one, got, 0, 5000, str(tmp_path / "b"))
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    ids = a["read_ids"].astype(np.int64)
    assert len(ids) == 700 and len(np.unique(ids)) == 700 and np.all(np.diff(ids) > 0)
    assert np.array_equal(a["read_type"], got.read_type[ids])
    off = got.bad_offsets.astype(np.int64)
    assert np.array_equal(np.diff(a["bad_offsets"]), (off[ids + 1] - off[ids]))
    want = np.concatenate([got.bad_regions[off[i]:off[i + 1]] for i in ids])
    assert np.array_equal(a["bad_regions"], want)

    # two ranks, reads [0, 2000) and [2000, 5000): the same files as one rank holding them all
    from yacrd_amd.engine import Result
    halves = [Result(got.bad_offsets[:2001], got.bad_regions[:int(got.bad_offsets[2000])], got.read_type[:2000]),
              Result(got.bad_offsets[2000:] - got.bad_offsets[2000], got.bad_regions[int(got.bad_offsets[2000]):],
                     got.read_type[2000:])]
    sent = {}

    class Gather:  # (torch.distributed's all_gather_object, the two ranks called one after the other)
        def __init__(self, rank):
            self.rank = rank

        def all_gather_object(self, out, obj):
            sent[self.rank] = obj
            out[:] = [sent.get(0), sent.get(1)]
    bench.dump_outputs(types.SimpleNamespace(dist=Gather(1), world=2, rank=1), halves[1], 2000, 5000, str(tmp_path / "r"))
    assert not os.path.exists(tmp_path / "r")  # (rank 0 writes)
    bench.dump_outputs(types.SimpleNamespace(dist=Gather(0), world=2, rank=0), halves[0], 0, 5000, str(tmp_path / "r"))
    r = load(tmp_path / "r")
    for k in a:
        assert np.array_equal(a[k], r[k]), k

    others = 8 * 700 + 4 * 700 + 8 * 701 + 8 * 5  # read_ids, read_type, bad_offsets, totals
    monkeypatch.setattr(bench, "DUMP_LIMIT", others + 4096 + 8 * 100)  # room for 100 regions only
    bench.dump_outputs(one, got, 0, 5000, str(tmp_path / "cut"))
    c = load(tmp_path / "cut")
    assert len(c["bad_regions"]) == 100 and np.array_equal(c["bad_regions"], a["bad_regions"][:100])
