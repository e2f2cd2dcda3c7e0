"""Pins tests/edit_fasta_window_cases.py — what tests/test_gpu_edit_fasta_windows.py compares the FASTA editor's run in
windows with — on the CPU: the generated texts' expected bytes are the host loop's and the restatement's, every generated
record fits the window the GPU tests use however it is laid out, the rule `windows_take` says True for every generated text
and False for the long-record and missing-newline cases, and the window-by-window restatement `window_carries` agrees with
the rule."""
import pytest

from edit_fasta_cases import OPS, _WIDTHS, device_takes, fallback_cases, host_loop, restate
from edit_fasta_window_cases import (MAX_BASES, W_SMALL, blank_front_text, filler, fillers, long_record_text, n_windows, record_of,
                                     record_spans, window_carries, window_cases, windows_take)


@pytest.fixture(scope="module")
def cases():
    return list(window_cases())


def test_expected_bytes_are_the_host_loops(cases, tmp_path):
    for tag, text, table in cases:
        for op in OPS:
            want, n_in, n_out = restate(text, op, table)
            assert host_loop(str(tmp_path), op, text, table, ext=".fasta") == want, (tag, op)
            assert n_in == len(record_spans(text)[1]) and n_out == want.count(b">") > 0  # (no description of the generator holds a '>')


def test_every_generated_record_fits_a_window(cases):
    """width 1 doubles a record's bytes, blank lines behind 15 % of its lines add two each on average: the table's longest
    read leaves room for both, and the generated records are measured"""
    assert 2 * MAX_BASES + MAX_BASES * 3 * 3 // 10 + 200 <= W_SMALL  # (twice the expected blank lines)
    for tag, text, table in cases:
        front, recs = record_spans(text)
        assert max(recs) <= W_SMALL and front <= W_SMALL, tag
        assert max(table.lengths) == MAX_BASES


def test_generated_texts_are_taken_and_cover_what_they_promise(cases):
    for tag, text, table in cases:
        assert len(text) >= 40 * W_SMALL and windows_take(text, W_SMALL) is True and n_windows(text, W_SMALL) >= 40, tag
        carries = window_carries(text, W_SMALL)
        assert carries is not None and len(carries) == n_windows(text, W_SMALL) - 1 and max(carries) > 1000
        for op in OPS:
            assert device_takes(text, table, op), (tag, op)
        lines = text.split(b"\n")
        heads = [l for l in lines if l.startswith(b">")]
        assert text.startswith(b"\n\n>") and b"\n\n\n" in text and b">f\n>" in text
        assert any(b"\t" in h for h in heads) and any(b"\x0c" in h for h in heads) and any(b" " in h for h in heads)
        assert any(h.endswith((b" ", b"\t", b"\x0c")) for h in heads) and any(h.isalnum() or b"/" in h for h in heads)
        keys = [h[1:].replace(b"\t", b" ").replace(b"\x0c", b" ").split(b" ")[0] for h in heads]
        assert any(k not in table.by_key for k in keys) and sum(k in table.by_key for k in keys) > len(keys) // 2
        body = {len(l) for l in lines if not l.startswith(b">")}
        assert {0, 1, 7, 60, 70, 80, 81} <= body and max(body) > 81 and len(body) > 60  # every width, one-line records, ragged lines
        assert None in _WIDTHS and "ragged" in _WIDTHS and 1 in _WIDTHS
    table = cases[0][2]
    assert len(table.names) == 2000 and set(table.types) == {0, 1, 2} and any(table.regions) and not all(table.regions)


def test_the_rule_on_long_records_and_missing_newlines(cases):
    W = W_SMALL
    assert windows_take(long_record_text(W), W) is False and window_carries(long_record_text(W), W) is None
    for at in (0, W + 1, 2 * W - 1):  # a record of exactly W bytes wherever it begins
        text = (fillers(at) if at else b"") + record_of(W) + filler(33)
        assert len(record_of(W)) == W and text[at:].startswith(b">big")
        assert windows_take(text, W) is True and window_carries(text, W) is not None, at
    assert windows_take(fillers(W) + record_of(W + 1) + filler(33), W) is None
    assert windows_take(fillers(W) + record_of(2 * W) + filler(33), W) is None
    text = cases[0][1]
    assert windows_take(text[:-1], W) is False and window_carries(text[:-1], W) is None
    assert windows_take(text + b">r", W) is False and window_carries(text + b">r", W) is None
    front = blank_front_text(W)
    assert record_spans(front)[0] == W + 1 + len(b">first one\n") and windows_take(front, W) is True
    assert window_carries(front, W) == [W] and n_windows(front, W) == 2
    assert windows_take(b"\n" * (2 * W) + b">r\nAC\n", W) is False and window_carries(b"\n" * (2 * W) + b">r\nAC\n", W) is None
    for tag, _, bad, _ in fallback_cases():  # (behind three good windows, as the GPU test appends them)
        late = fillers(3 * W) + bad
        assert windows_take(late, W) is (False if tag.startswith("no_final_newline") else True), tag


def test_a_complete_record_at_a_windows_end_is_deferred():
    """nothing in a window says that the next byte is '>': the record that ends with the window is carried whole"""
    W = 4096
    text = fillers(W - 700) + record_of(700, b"ends") + fillers(W // 2)
    assert text[W:W + 2] == b">f" and text[W - 1:W] == b"\n"
    assert window_carries(text, W) == [700]


def test_the_two_restatements_agree():
    """wherever the rule says True the window-by-window run goes through, wherever it says False it does not"""
    W = 4096
    for size in (100, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W):
        for at in (0, 1000, W - 1, W, W + 7):
            for width in (80, 1):
                text = (fillers(at) if at else b"") + record_of(size, width=width) + fillers(2 * W + 5)
                took, carries = windows_take(text, W), window_carries(text, W)
                assert took is not False or carries is None, (size, at)
                assert took is not True or carries is not None, (size, at)
