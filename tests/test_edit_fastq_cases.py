"""Pins tests/edit_fastq_cases.py — what tests/test_gpu_edit_fastq.py compares the device FASTQ editor with — to the
yardsticks, on the CPU: the restated rules equal the host loop (yacrd_edit_file) on every case and all four ops, equal
oracle/editors.py where that applies, and the predicate `device_takes` sorts the two sets the way the interface says."""
import pytest

import oracle
from oracle import editors as oracle_editors
from edit_fastq_cases import (OPS, OP_NAMES, OP_SCRUBB, OP_SPLIT, Table, cut_pairs, device_takes, fallback_cases, fuzz_cases, host_loop,
                              oracle_table, restate)


@pytest.fixture(scope="module")
def cases():
    return list(fuzz_cases())


def test_restatement_is_the_host_loop_on_every_case(cases, tmp_path):
    n = 0
    for tag, text, table in cases:
        for op in OPS:
            want, n_in, n_out = restate(text, op, table)
            assert host_loop(str(tmp_path), op, text, table) == want, (tag, op)
            assert n_in == text.count(b"\n") // 4 and n_out == want.count(b"\n") // 4
        n += 1
    assert n >= 250


def test_the_chunk_parallel_host_loop_agrees(cases, tmp_path):
    for tag, text, table in cases[::16]:
        for op in OPS:
            assert host_loop(str(tmp_path), op, text, table, n_threads=3) == restate(text, op, table)[0], (tag, op)


def test_restatement_is_the_oracle_where_it_applies(cases):
    n = 0
    for tag, text, table in cases:
        ot = oracle_table(table)
        if ot is None:
            continue
        for op in OPS:
            assert oracle_editors.edit_fastq(OP_NAMES[op], text, ot, 0.4) == restate(text, op, table)[0], (tag, op)
        n += 1
    assert n >= 100


def test_the_cases_cover_what_they_promise(cases):
    tables = [t for _, _, t in cases]
    ids = [n for t in tables for n in t.names]
    assert min(map(len, ids)) == 1 and max(map(len, ids)) == 300
    assert any(a != b and b.startswith(a) for t in tables for a in t.names for b in t.names)
    assert {ty for t in tables for ty in t.types} == {0, 1, 2}
    digits = {len(str(p)) for t in tables for r in t.regions for pair in r for p in pair}
    assert digits >= {1, 2, 3, 4, 5, 6, 7}
    heads = [l for _, text, _ in cases for l in text.split(b"\n")[0::4] if l]
    assert any(b" " in h for h in heads) and any(b" " not in h for h in heads) and any(b"\t" in h for h in heads)
    seqs = {len(l) for _, text, _ in cases for l in text.split(b"\n")[1::4]}
    assert {0, 1} <= seqs and max(seqs) >= 100000
    absent = sum(1 for _, text, t in cases for h in text.split(b"\n")[0::4] if h and h[1:].split(b" ")[0].split(b"\t")[0] not in t.by_key)
    assert absent > len(heads) // 6
    # a zero-length piece, a read that vanishes, a single region over everything
    assert any(p0 == p1 for t in tables for r, l in zip(t.regions, t.lengths) for p0, p1 in cut_pairs(OP_SCRUBB, r, l))
    assert any(r and not cut_pairs(OP_SCRUBB, r, l) for t in tables for r, l in zip(t.regions, t.lengths))
    assert any(r == [(0, l)] and l for t in tables for r, l in zip(t.regions, t.lengths))


def test_cut_pairs_on_the_reference_shapes():
    assert cut_pairs(OP_SCRUBB, [(0, 5), (20, 30)], 40) == [(5, 20), (30, 40)]      # a leading 0,0 pair is skipped
    assert cut_pairs(OP_SCRUBB, [(5, 10), (30, 40)], 40) == [(0, 5), (10, 30)]      # len already last: the odd element is ignored
    assert cut_pairs(OP_SCRUBB, [(0, 40)], 40) == []                                # the read vanishes
    assert cut_pairs(OP_SCRUBB, [(3, 5), (5, 9)], 12) == [(0, 3), (5, 5), (9, 12)]  # adjacent regions: a zero-length piece
    assert cut_pairs(OP_SPLIT, [(0, 5), (20, 30), (35, 40)], 40) == [(0, 20), (30, 40)]  # only the middle regions
    assert cut_pairs(OP_SPLIT, [], 40) == [(0, 40)]


def test_device_takes_sorts_the_two_sets(cases):
    for tag, text, table in cases:
        for op in OPS:
            assert device_takes(text, table, op), (tag, op)
    seen = set()
    for tag, ops, text, table in fallback_cases():
        for op in OPS:
            assert device_takes(text, table, op) == (op not in ops), (tag, op)
        seen.add(tag)
    assert {"crlf", "plus_name", "blank_line", "no_final_newline", "lengths_differ", "bare_at", "blank_before_newline", "fifth_line",
            "position_beyond_read", "begin_after_end"} <= seen
    assert oracle.NOT_BAD == 0 and Table().get(b"x") == ([], 0, 0)
