"""Pins tests/edit_fasta_cases.py — what tests/test_gpu_edit_fasta.py compares the device FASTA editor with — to the yardstick,
on the CPU: the restated rules equal the host loop (yacrd_edit_file on a ".fasta") on every case and all four ops, one-thread
and chunk-parallel; the predicate `device_takes` sorts the two sets the way the interface says; and the interface itself is
declared: the header and the Python binding name the four calls."""
import os
import re

import pytest

from edit_fasta_cases import (BASES_FIRST, OPS, OP_SCRUBB, Table, cut_pairs, device_takes, fallback_cases, fuzz_cases, host_loop, restate, wrap,
                              _records, _split_header)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["yacrd_engine_edit_fasta", "yacrd_engine_edit_fasta_mem", "yacrd_engine_edit_fasta_gzip_mem", "yacrd_engine_edit_fasta_gzip_file"]


@pytest.fixture(scope="module")
def cases():
    return list(fuzz_cases())


def test_restatement_is_the_host_loop_on_every_case(cases, tmp_path):
    n = 0
    for tag, text, table in cases:
        for op in OPS:
            want, n_in, n_out = restate(text, op, table)
            assert host_loop(str(tmp_path), op, text, table, ext=".fasta") == want, (tag, op)
            assert n_in == sum(1 for l in text.split(b"\n") if l.startswith(b">")) and n_out == len(_records(want))
        n += 1
    assert n >= 150


def test_the_chunk_parallel_host_loop_agrees(cases, tmp_path, monkeypatch):
    monkeypatch.setenv("YACRD_EDIT_CHUNK", "64")
    for tag, text, table in cases:
        for op in OPS:
            assert host_loop(str(tmp_path), op, text, table, ext=".fasta", n_threads=4) == restate(text, op, table)[0], (tag, op)


def test_the_host_loop_on_what_the_device_leaves_to_it(tmp_path):
    """a last line without its newline is read as a line; an empty name is written back as it stands; a line that is not blank
    in front of the first header is an error"""
    from yacrd_amd import host
    t = Table()
    assert host_loop(str(tmp_path), OP_SCRUBB, b">r d\nACGT\nAC", t, ext=".fasta") == b">r d\nACGTAC\n" == restate(b">r d\nACGT\nAC", OP_SCRUBB, t)[0]
    for text in (b">\nAC\n", b"> d\nAC\n"):
        assert host_loop(str(tmp_path), OP_SCRUBB, text, t, ext=".fasta") == text == restate(text, OP_SCRUBB, t)[0]
    for text in BASES_FIRST:
        with pytest.raises(host.HostError, match="fasta format failed"):
            host_loop(str(tmp_path), OP_SCRUBB, text, t, ext=".fasta")
        with pytest.raises(ValueError):
            restate(text, OP_SCRUBB, t)


def test_the_cases_cover_what_they_promise(cases):
    tables = [t for _, _, t in cases]
    ids = [n for t in tables for n in t.names]
    assert min(map(len, ids)) == 1 and max(map(len, ids)) == 300
    assert any(a != b and b.startswith(a) for t in tables for a in t.names for b in t.names)
    assert {ty for t in tables for ty in t.types} == {0, 1, 2}
    recs = [(h, s, text) for _, text, _ in cases for h, s in _records(text)]
    assert {0, 1, 79, 80, 81, 159, 160, 161, 200, 1000} <= {len(s) for _, s, _ in recs} and max(len(s) for _, s, _ in recs) >= 1200000
    assert any(10000 <= len(s) <= 100000 for _, s, _ in recs)
    heads = [h for h, _, _ in recs]
    for sep in (b" ", b"\t", b"\x0c"):
        assert any(_split_header(h)[0] + sep == h for h in heads), sep             # an empty description behind the separator
        assert any(h[len(_split_header(h)[0]):][:1] == sep and _split_header(h)[1] for h in heads), sep
    assert any(re.search(rb"[ \t\x0c]", _split_header(h)[1]) for h in heads) and any(b">" in h for h in heads)
    texts = [text for _, text, _ in cases]
    assert any(t.startswith(b"\n") for t in texts) and any(t.endswith(b"\n\n") for t in texts)
    assert any(re.search(rb"[ACGT]\n\n+[ACGT]", t) for t in texts)                   # a blank line inside a sequence
    assert any(re.search(rb"\n>[^\n]*\n>", t) for t in texts)                        # a record with no sequence line at all
    widths = {len(l) for t in texts if len(t) < 100000 for l in t.split(b"\n") if l and not l.startswith(b">")}
    assert {1, 7, 60, 70, 80, 81} <= widths and max(widths) > 90
    absent = sum(1 for (h, _, _), t in ((r, tb) for _, text, tb in cases for r in [(h, s, text) for h, s in _records(text)]) if _split_header(h)[0] not in t.by_key)
    assert absent > len(heads) // 6
    longer = sum(1 for _, text, tb in cases for h, s in _records(text) if _split_header(h)[0] in tb.by_key and len(s) > tb.get(_split_header(h)[0])[1])
    assert longer > 10
    assert any(p0 == p1 for t in tables for r, l in zip(t.regions, t.lengths) for p0, p1 in cut_pairs(OP_SCRUBB, r, l))


def test_wrap():
    assert wrap(b"") == b"" and wrap(b"A") == b"A\n" and wrap(b"A" * 80) == b"A" * 80 + b"\n"
    assert wrap(b"A" * 81) == b"A" * 80 + b"\nA\n" and wrap(b"A" * 160).count(b"\n") == 2


def test_device_takes_sorts_the_two_sets(cases):
    for tag, text, table in cases:
        for op in OPS:
            assert device_takes(text, table, op), (tag, op)
    seen = set()
    for tag, ops, text, table in fallback_cases():
        for op in OPS:
            assert device_takes(text, table, op) == (op not in ops), (tag, op)
        seen.add(tag)
    assert {"crlf", "lone_cr", "no_final_newline", "bare_mark", "no_name", "position_beyond_read", "begin_after_end"} <= seen
    for text in BASES_FIRST:
        assert not device_takes(text, Table(), OP_SCRUBB)


def test_the_interface_declares_the_four_calls():
    """the C header declares them, the Python binding lists them and gives the engine its three methods"""
    header = open(os.path.join(ROOT, "include", "yacrd_engine.h")).read()
    binding = open(os.path.join(ROOT, "yacrd_amd", "engine.py")).read()
    for call in CALLS:
        assert re.search(r"\bint %s\(yacrd_engine \*e, int op," % call, header), call
        assert '"%s"' % call in binding, call
    assert re.search(r"#define YACRD_ABI_VERSION 7\b", header)
    import yacrd_amd
    for method in ("edit_fasta", "edit_fasta_text", "edit_fasta_gzip"):
        assert callable(getattr(yacrd_amd.Engine, method))
