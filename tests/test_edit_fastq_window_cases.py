"""Pins tests/edit_fastq_window_cases.py — what tests/test_gpu_edit_fastq_windows.py compares the FASTQ editor's run in
windows with — on the CPU: the generated texts' expected bytes are the host loop's and the restatement's, the rule
`windows_take` says True for every generated text at the window the GPU tests use and False for the long-record and
missing-line cases, and the window-by-window restatement `window_carries` agrees with the rule."""
import pytest

from edit_fastq_cases import OPS, device_takes, fallback_cases, host_loop, restate
from edit_fastq_window_cases import (W_SMALL, filler, fillers, long_record_text, missing_line_texts, record_of, window_carries, window_cases,
                                     windows_take)


@pytest.fixture(scope="module")
def cases():
    return list(window_cases())


def test_expected_bytes_are_the_host_loops(cases, tmp_path):
    for tag, text, table in cases:
        for op in OPS:
            want, n_in, n_out = restate(text, op, table)
            assert host_loop(str(tmp_path), op, text, table) == want, (tag, op)
            assert n_in == text.count(b"\n") // 4 and n_out == want.count(b"\n") // 4 and n_out > 0


def test_generated_texts_are_taken_and_cover_what_they_promise(cases):
    for tag, text, table in cases:
        assert len(text) >= 40 * W_SMALL and windows_take(text, W_SMALL) is True, tag
        carries = window_carries(text, W_SMALL)
        assert carries is not None and len(carries) == (len(text) + W_SMALL - 1) // W_SMALL - 1 and max(carries) > 1000
        for op in OPS:
            assert device_takes(text, table, op), (tag, op)
        lines = text.split(b"\n")
        heads, seqs, quals = lines[0:-1:4], lines[1::4], lines[3::4]
        assert b"@f\n\n+\n\n" in text and {0, 3000} <= {len(s) for s in seqs}
        assert any(q.startswith(b"@") for q in quals) and any(q.startswith(b"+") for q in quals)
        assert any(b" " in h for h in heads) and any(b" " not in h for h in heads)
        keys = [h[1:].split(b" ")[0] for h in heads]
        assert any(k not in table.by_key for k in keys) and sum(k in table.by_key for k in keys) > len(keys) // 2
    table = cases[0][2]
    assert len(table.names) == 2000 and set(table.types) == {0, 1, 2} and any(table.regions) and not all(table.regions)


def test_the_rule_on_long_records_and_missing_lines(cases):
    W = W_SMALL
    assert windows_take(long_record_text(W), W) is False and window_carries(long_record_text(W), W) is None
    for at in (0, W + 1, 2 * W - 1):  # a record of exactly W bytes wherever it begins
        text = (fillers(at) if at else b"") + record_of(W) + filler(33)
        assert windows_take(text, W) is True and window_carries(text, W) is not None, at
    assert windows_take(fillers(W) + record_of(W + 1) + filler(33), W) is None
    assert windows_take(fillers(W) + record_of(2 * W) + filler(33), W) is None
    text = cases[0][1]
    for tag, broken in missing_line_texts(text, W):
        assert windows_take(broken, W) is False and window_carries(broken, W) is None, tag
    for tag, _, bad, _ in fallback_cases():  # (behind three good windows, as the GPU test appends them)
        late = fillers(3 * W) + bad
        assert windows_take(late, W) is (False if tag in ("blank_line", "no_final_newline", "fifth_line") else True), tag


def test_the_two_restatements_agree():
    """wherever the rule says True the window-by-window run goes through, wherever it says False it does not"""
    W = 4096
    for size in (100, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W):
        for at in (0, 1000, W - 1, W, W + 7):
            text = (fillers(at) if at else b"") + record_of(size) + fillers(2 * W + 5)
            took, carries = windows_take(text, W), window_carries(text, W)
            assert took is not False or carries is None, (size, at)
            assert took is not True or carries is not None, (size, at)
