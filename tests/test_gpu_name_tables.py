"""The device's name tables under crafted probe chains: ids that all home into the last 256 slots of the table
(tests/name_table_cases.py), so that a chain of hundreds of slots runs across the table's last slot, misses end at the chain's
far end, and the device parser's bounded walk and capacity rule are met exactly.  None of these inputs is meant to fault
anything: each ends in a result or in NeedsHostParser.  The yardsticks are the suite's own — the host parser and the oracle
for an ingest, the host loop and the restatements for the editors, the host reader for a report — never the device path."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import edit_fasta_cases as fa
import edit_fastq_cases as fq
import name_table_cases as nt
import oracle
import report_cases as rc
import yacrd_amd
from cases import assert_same
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, host_loop as overlaps_host_loop, restate as overlaps_restate
from input_csr_cases import assert_same_csr
from yacrd_amd import host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "yacrd_amd", "bin", "yacrd")
FULL = "more read ids than the device table holds"
FORMATS = [(1, ".paf"), (2, ".m4")]
FORMAT_IDS = ["paf", "m4"]


@pytest.fixture(scope="module")
def engine():
    with yacrd_amd.Engine(device_id=0) as e:
        yield e


# ---- the device parser, one engine ---------------------------------------------------------------------------------------------------
def _taken(engine, text, fmt, cov=2, nc=0.4, python_ingest=False, what=""):
    """`text` is parsed on the device (NeedsHostParser propagates) and everything equals the host parser + the oracle; with
    `python_ingest` the names and the CSR also equal the oracle's own ingest (small texts)"""
    got, names, lengths, stats = engine.ingest_text(text, cov, nc, fmt=fmt)
    c = host.csr_from_memory(text, fmt, n_threads=4)
    assert names == c.names, what + ": names in first-appearance order"
    assert np.array_equal(lengths, c.lengths), what + ": first length seen"
    assert stats["n_reads"] == len(c.names) and stats["n_records"] == c.n_records == text.count(b"\n")
    assert_same_csr(engine.debug_input_csr(), (c.offsets, c.intervals, c.lengths), what)
    if python_ingest:
        reads = (oracle.parse_m4 if fmt == 2 else oracle.parse_paf)(text.decode())
        w_names, off, iv, ln = oracle.to_csr(reads)
        assert names == list(w_names) and np.array_equal(lengths.astype(np.uint64), ln)
        assert_same_csr((c.offsets, c.intervals, c.lengths), (off, iv, ln), what + ": host parser vs oracle ingest")
    assert_same(got, oracle.run(c.offsets, c.intervals, c.lengths.astype(np.uint64), cov, nc, n_threads=4), what)
    return names


def _falls_back(engine, text, fmt, comfortably):
    with pytest.raises(yacrd_amd.NeedsHostParser) as x:
        engine.ingest_text(text, 2, 0.4, fmt=fmt)
    assert FULL in str(x.value) and ("comfortably" in str(x.value)) == comfortably, str(x.value)
    assert engine.debug_input_csr() is None  # a failed call leaves no CSR to show


def _chain_is_taken(engine, fmt):
    ids = nt.chain_ids()
    names = _taken(engine, nt.overlap_text(ids, fmt == 2), fmt, python_ingest=True, what="900 pool ids and 50 plain ones")
    assert sorted(names) == sorted(x.decode() for x in ids)


@pytest.mark.parametrize("fmt,ext", FORMATS, ids=FORMAT_IDS)
def test_a_chain_of_900_slots_across_the_tables_end_is_taken(engine, fmt, ext):
    """(a) 900 pool ids occupy one block of 900 slots that starts in the last 256 of 2^20 and crosses slot 2^20 - 1; no walk is
    longer than the block in any insertion order (tests/test_name_table_cases.py), so the parse must not fall back."""
    _chain_is_taken(engine, fmt)


@pytest.mark.parametrize("fmt,ext", FORMATS, ids=FORMAT_IDS)
def test_b_1400_ids_in_one_chain_outgrow_the_bounded_walk(engine, fmt, ext):
    """(b) Only 1400 reads, far below the capacity rule, but all in one chain: in every insertion order the id that ends in
    the block's last slot has looked at 1400 - 255 = 1145 > 1025 slots, so gp_intern gives up and the file is the host
    parser's.  This case also proves that the hash restated in name_table_cases.py IS the device's: with a wrong restatement
    the ids would scatter over 2^20 slots, the file would be taken and the test would fail.  Afterwards the same engine shows
    no CSR and takes case (a) again: the table is reset after a failed call."""
    ids = nt.pool(1400)
    assert nt.parser_holds_comfortably(len(ids), nt.PARSER_MIN_CAP)
    _falls_back(engine, nt.overlap_text(ids, fmt == 2), fmt, comfortably=False)
    _chain_is_taken(engine, fmt)


@pytest.fixture(scope="module")
def walk_texts():
    return {walk: nt.walk_case(walk) for walk in (nt.WALK_SLOTS, nt.WALK_SLOTS + 1)}


def test_b_a_walk_of_1025_slots_is_taken_and_one_of_1026_is_not(engine, walk_texts):
    """(b), to the slot.  The parse is launched once per 128 MiB: the ids of the first launch fill a block, and ONE id named
    only behind byte 128 MiB walks from its home to the block's end, a number of slots that no insertion order changes
    (name_table_cases.walk_case).  1025 slots — the last one empty — is what gp_intern looks at: taken, and equal to host +
    oracle.  1026 slots: kTableFull, with two reads more than before."""
    text, K, x = walk_texts[nt.WALK_SLOTS]
    names = _taken(engine, text, 1, what="a walk of %d slots" % nt.WALK_SLOTS)
    assert len(names) == K + 2 and names[-1] == x.decode()
    text, K1, _ = walk_texts[nt.WALK_SLOTS + 1]
    assert K1 == K + 1
    _falls_back(engine, text, 1, comfortably=False)
    _chain_is_taken(engine, 1)


def _small_text_is_taken(engine):
    text = b"a\t100\t1\t50\t+\tb\t200\t2\t60\nb\t200\t3\t70\t-\tc\t300\t4\t80\n"
    assert _taken(engine, text, 1, cov=0, nc=0.8, python_ingest=True, what="a small text afterwards") == ["a", "b", "c"]


def test_c_the_capacity_rule_at_its_edge(engine):
    """(c) 2 R > cap at cap = 2^20: 524 288 plain ids are taken (their longest cluster has a few dozen slots: pinned on the
    CPU), one more falls back with "holds comfortably"; 1 100 000 ids, more than there are slots, fill the table and fall back
    from the walk.  After each fallback the engine takes a small text."""
    text = nt.distinct_text(524288)
    assert nt.parser_cap(len(text)) == nt.PARSER_MIN_CAP and text.count(b"\n") == 262144
    names = _taken(engine, text, 1, what="524288 ids")
    assert len(names) == 524288 and names[:3] == ["r0", "r1", "r2"] and names[-1] == "r7ffff"
    text = nt.distinct_text(524289)
    assert nt.parser_cap(len(text)) == nt.PARSER_MIN_CAP
    _falls_back(engine, text, 1, comfortably=True)
    _small_text_is_taken(engine)
    text = nt.distinct_text(1100000)
    assert nt.parser_cap(len(text)) == nt.PARSER_MIN_CAP < 1100000
    _falls_back(engine, text, 1, comfortably=False)
    _small_text_is_taken(engine)


def _lines(path):
    with open(path) as f:
        return [l.rstrip("\n") for l in f]


def test_d_a_read_to_reference_paf_through_the_cli(tmp_path):
    """(d) A new query id on every line: 600 001 reads.  The device parse runs to its end, comes back as YACRD_EFALLBACK, and
    the CLI goes on with the host parser: the oracle's report on the host parser's CSR, no "[info] device parser:" line, and
    the bytes of a run that never tried the device parser."""
    paf = str(tmp_path / "r2r.paf")
    with open(paf, "wb") as f:
        f.write(nt.read_to_reference(600000))
    assert nt.parser_cap(os.path.getsize(paf)) == nt.PARSER_MIN_CAP
    outs = []
    for k, env in enumerate(({}, {"YACRD_NO_DEVICE_PARSER": "1"})):
        out = str(tmp_path / ("out%d.yacrd" % k))
        p = subprocess.run([BIN, "-i", paf, "-o", out, "-c", "1", "-n", "0.4"], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, YACRD_CLI_TIMING="1", **env))
        assert p.returncode == 0, p.stdout + p.stderr
        assert "[info] device parser:" not in p.stderr, p.stderr
        with open(out, "rb") as f:
            outs.append(f.read())
    assert outs[0] == outs[1] and outs[0]
    c = host.csr_from_file(paf, n_threads=4)
    assert len(c.names) == 600001 and c.names[1] == "ref"
    ln = c.lengths.astype(np.uint64)
    bo, br, rt = oracle.run(c.offsets, c.intervals, ln, 1, 0.4, n_threads=4)
    want = oracle.report_from_csr(c.names, ln, bo, br, rt)
    got = _lines(str(tmp_path / "out0.yacrd"))
    assert len(got) == 600001 and set(got) == set(want)


# ---- the merge table, N engines on one device -------------------------------------------------------------------------------------
_MERGE = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import oracle, yacrd_amd
import name_table_cases as nt
from cases import assert_same
from input_csr_cases import assert_same_csr, assert_same_csr_in_ranges
from test_gpu_ingest_group import _same_ingest
# YACRD_TEST_RANGE_BYTES=32768 (this process): a text of N * 32 KiB is cut into N ranges of 32 KiB
pool = nt.pool(305)
engines = [yacrd_amd.Engine() for _ in range(3)]
for n, late in ((2, []), (3, []), (2, pool[300:305]), (3, pool[300:305])):
    text = nt.merge_text(n, pool[:300], late)
    cuts = nt.range_cuts(len(text), n)
    M = sum(len(s) for s in nt.ids_per_range(text, cuts))  # the merge's entries: a read once per range that names it
    assert M == 300 * n + len(late) and nt.pow2_cap(M) == 2048
    what = "%d engines, %d late ids" % (n, len(late))
    one = engines[0].ingest_text(text, 2, 0.4)
    w_names, off, iv, ln = oracle.to_csr(oracle.parse_paf(text.decode()))
    assert one[1] == list(w_names) and np.array_equal(one[2].astype(np.uint64), ln) and len(w_names) == 300 + len(late)
    assert_same_csr(engines[0].debug_input_csr(), (off, iv, ln), what + ": one engine")
    assert_same(one[0], oracle.run(off, iv, ln, 2, 0.4, n_threads=2), what + ": one engine vs oracle")
    got = yacrd_amd.ingest_overlaps(engines[:n], text, 2, 0.4)
    _same_ingest(got, one, what)
    assert_same_csr_in_ranges([e.debug_input_csr() for e in engines[:n]], (off, iv, ln), what)
    print("MERGE", n, len(late), M, flush=True)
print("MERGE OK")
"""


def test_merge_table_holds_every_ranges_chain(tmp_path):
    """N engines on one device, the ranges cut every 32 KiB (YACRD_TEST_RANGE_BYTES, read once per process: a child).  Every
    range names all of 300 pool ids, so the merge table of 2048 slots takes M = 300 N entries that home into its last 256
    slots: N entries per read in one chain across the table's end, every one of which must find its read's slot.  A second
    text has five ids that only the last range names."""
    script = tmp_path / "merge.py"
    script.write_text(_MERGE)
    p = subprocess.run([sys.executable, str(script), ROOT], env=dict(os.environ, YACRD_TEST_RANGE_BYTES=str(nt.RANGE_BYTES)),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert p.stdout.splitlines()[-1] == "MERGE OK" and p.stdout.count("MERGE ") == 5, p.stdout[-2000:]


# ---- the editors' table ---------------------------------------------------------------------------------------------------------
TABLES = [(True, nt.small_table), (False, nt.large_table)]
TABLE_IDS = ["400_ids_1024_slots", "1400_ids_4096_slots"]


@pytest.mark.parametrize("small,table", TABLES, ids=TABLE_IDS)
@pytest.mark.parametrize("fmt,ext", FORMATS, ids=FORMAT_IDS)
def test_overlap_editors_find_and_miss_inside_the_chain(engine, tmp_path, fmt, ext, small, table):
    names, types = table()
    text = nt.overlap_text(nt.lookup_ids(names, small), fmt == 2)
    by_name = dict(zip(names, types))
    for op in (OP_FILTER, OP_EXTRACT):
        got = engine.edit_overlaps_text(op, text, names, types, fmt)  # (raises on YACRD_EFALLBACK)
        want, n_lines, n_kept = overlaps_restate(text, op, by_name, fmt == 2)
        assert 0 < n_kept < n_lines
        assert got == overlaps_host_loop(str(tmp_path), op, text, names, types, ext), (op, fmt)
        assert got == want, (op, fmt)
        st = engine.edit_stats
        assert (st["kept_bytes"], st["n_kept"], st["n_lines"], st["text_bytes"]) == (len(want), n_kept, n_lines, len(text))


def _seq_table(names, types):
    """the report table of a sequence editor over the name table's ids: lengths and regions of the shapes the editors' own
    cases use (edit_fastq_cases._regions), types as the name table mixes them"""
    rng = random.Random(len(names))
    lengths = [rng.choice([0, 1, 11, 60, 100, 161]) for _ in names]
    regions = [fq._regions(rng, fq._SHAPES[i % len(fq._SHAPES)], n) for i, n in enumerate(lengths)]
    return fq.Table(names, lengths, regions, types)


def _seq_text(table, ids, fasta):
    """one record per id of `ids`, in an order of its own: a sequence as long as the table says, 30 bases for an id it does not
    hold; every third header carries a description"""
    rng = random.Random(7 * len(ids))
    order = list(ids)
    rng.shuffle(order)
    out = []
    for k, x in enumerate(order):
        _, length, _ = table.get(x)
        n = length if x in table.by_key else 30
        seq = bytes(rng.choice(b"ACGT") for _ in range(n))
        head = x + (b" d%d x" % k if k % 3 == 0 else b"")
        if fasta:
            out.append(b">" + head + b"\n" + fa.lay_out(rng, seq, (60, 80, None)[k % 3]))
        else:
            out.append(b"@" + head + b"\n" + seq + b"\n+\n" + bytes(33 + (k + j) % 90 for j in range(n)) + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("small,table", TABLES, ids=TABLE_IDS)
@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
def test_sequence_editors_find_and_miss_inside_the_chain(engine, tmp_path, fasta, small, table):
    names, types = table()
    t = _seq_table(names, types)
    text = _seq_text(t, nt.lookup_ids(names, small), fasta)
    mod, ext = (fa, ".fasta") if fasta else (fq, ".fastq")
    t_names, lengths, bo, br, rt = t.arrays()
    for op in fq.OPS:
        assert mod.device_takes(text, t, op)
        got = (engine.edit_fasta_text if fasta else engine.edit_fastq_text)(op, text, t_names, lengths, (bo, br, rt))
        want, n_in, n_out = mod.restate(text, op, t)
        assert got == fq.host_loop(str(tmp_path), op, text, t, ext=ext), (op, fasta)
        assert got == want, (op, fasta)
        assert 0 < n_out and n_in == len(nt.lookup_ids(names, small))
        st = engine.seq_edit_stats
        assert (st["text_bytes"], st["out_bytes"], st["n_records"], st["n_out_records"]) == (len(text), len(want), n_in, n_out)


# ---- the report reader ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ids,n_dup,cap", [(400, 100, 1024), (1400, 400, 4096)])
def test_report_reader_dedupes_inside_the_chain(engine, tmp_path, n_ids, n_dup, cap):
    """a report over pool ids, some of them again further down: the first position is kept and the last values win (as
    test_duplicates_keep_the_first_position_and_the_last_values states it), equal to the host reader, with no fallback"""
    ids = nt.pool(n_ids)
    text = nt.report_rows(ids, n_dup)
    assert nt.pow2_cap(text.count(b"\n")) == cap
    want = rc.host_read(tmp_path, text)
    assert rc.same(want, rc.restate(text))
    assert want[0] == ids  # first positions: the duplicates add no read and move none
    assert want[1][3] == 5000  # report_rows' first duplicate is of id 3, and its only one: the duplicate's length
    got_res, got_names, got_lengths, stats = engine.ingest_report(text, 0.4)  # (raises on YACRD_EFALLBACK)
    got = ([s.encode("utf-8", "surrogateescape") for s in got_names], got_lengths, got_res.bad_offsets, got_res.bad_regions)
    assert rc.same(got, want)
    assert stats["n_reads"] == n_ids and stats["n_records"] == n_ids + n_dup
    assert np.array_equal(got_res.read_type, engine.classify(want[2], want[3], want[1], 0.4))
