"""The yardsticks of tests/test_gpu_edit_bgzf_windows.py pinned without a GPU (tests/edit_bgzf_window_cases.py): the run
restated for windows that end anywhere equals the two existing restatements where the windows end at multiples of W; the
stream builders give streams the host decoder and zlib read back as the text, cut where member_cuts says; and the bytes the
GPU tests expect — restate — are the host loop's."""
import gzip
import os
import random
import shutil
import subprocess

import pytest

import edit_fasta_cases as fa
import edit_fasta_window_cases as faw
import edit_fastq_cases as fq
import edit_fastq_window_cases as fqw
from edit_bgzf_window_cases import (ISIZES, W_BGZF, borders_of, check_cut_properties, cuts_of, drawn_sizes, drawn_stream, frames_of,
                                    stream_of, window_carries_at)
from inflate_cases import write_check_file, zlib_says
from yacrd_amd import host

W = W_BGZF


def _borders(text, w):
    return [min(len(text), (k + 1) * w) for k in range((len(text) + w - 1) // w)]


@pytest.fixture(scope="module")
def texts():
    """(fasta?, tag, text, table): the generated texts of the GPU tests, 20 windows of W each"""
    out = []
    t = fqw.window_table()
    out += [(False, "fastq gen%d" % k, fqw.window_text(t, 1000 + k, 20 * W), t) for k in range(2)]
    t = faw.window_table()
    out += [(True, "fasta gen%d" % k, faw.window_text(t, 2000 + k, 20 * W), t) for k in range(2)]
    return out


def test_borders_at_multiples_of_w_give_the_existing_restatements(texts):
    for fasta, tag, text, _ in texts:
        mod = faw if fasta else fqw
        for w in (32768, W, 100000):
            want = mod.window_carries(text, w)
            assert want is not None and window_carries_at(text, _borders(text, w), fasta, w) == want, (tag, w)
    # and where the run does not go through: a record of 2 W + 1, chains of W + 15, a missing last newline, a missing line
    for fasta, mod in ((False, fqw), (True, faw)):
        for w in (32768, W):
            odd = [mod.long_record_text(w), mod.fillers(w - 5) + b"".join(mod.record_of(w + 15, b"c%02d" % i) for i in range(8)) + mod.filler(55),
                   mod.fillers(w + 15) + b"".join(mod.record_of(w - 5, b"c%02d" % i) for i in range(8)) + mod.filler(55),
                   mod.fillers(3 * w + 100)[:-1]]
            for text in odd:
                assert window_carries_at(text, _borders(text, w), fasta, w) == mod.window_carries(text, w), (fasta, w, len(text))
    text = fqw.fillers(5 * W)
    for tag, bad in fqw.missing_line_texts(text, W):
        assert window_carries_at(bad, _borders(bad, W), False, W) is None and fqw.window_carries(bad, W) is None, tag


def test_windows_that_bring_nothing(texts):
    """a border repeated — a window with no new byte — changes no carry but its own, which is the one before again"""
    for fasta, tag, text, _ in texts:
        b = _borders(text, W)
        base = window_carries_at(text, b, fasta, W)
        twice = window_carries_at(text, b[:3] + [b[2]] + b[3:], fasta, W)
        assert twice == base[:3] + [base[2]] + base[3:], tag
        end = window_carries_at(text, b + [b[-1]], fasta, W)
        # a last window of no bytes: FASTQ's text ended whole; FASTA's last record waited, and that window completes it
        assert end == base + [len(text) - text.rindex(b"\n>") - 1 if fasta else 0], tag


def test_the_builders_give_the_text_back(texts):
    rng = random.Random(3)
    assert set(ISIZES) <= set(s for k in range(40) for s in drawn_sizes(random.Random(k), 600000))
    for fasta, tag, text, _ in texts[::2]:
        blob, sizes = drawn_stream(text, 11)
        isizes, frames = frames_of(blob)
        assert isizes == sizes + [0] and max(frames) <= 65536
        assert zlib_says(blob) == text and host.bgzf_decode_host(blob) == text and gzip.decompress(blob) == text, tag
        cuts = cuts_of(blob, W)
        check_cut_properties(cuts, isizes, frames, W)
        assert cuts == host.bgzf_window_cuts(blob, W) and len(cuts) >= 20
        assert window_carries_at(text, borders_of(cuts), fasta, W) is not None, tag
    for kind in ("stored", "level1", "level6"):
        text = bytes(rng.randrange(65, 91) for _ in range(70000))
        assert zlib_says(stream_of(text, [0, 1, 65536, 0, 4463, 0], kind)) == text


def test_the_expected_bytes_are_the_host_loops(texts, tmp_path):
    """restate — what the GPU tests compare with — against host.edit_file on the same plain text"""
    for fasta, tag, text, table in texts[::2]:
        mod, ext = (fa, ".fasta") if fasta else (fq, ".fastq")
        for op in (fq.OP_SCRUBB, fq.OP_SPLIT):
            want = mod.restate(text, op, table)[0]
            d = tmp_path / ("%s_%d" % (ext[1:], op))
            d.mkdir()
            assert want == fq.host_loop(str(d), op, text, table, ext=ext), (tag, op)


def test_the_last_byte_before_the_first_window_under_the_sanitizers(texts, tmp_path):
    """what a BGZF run in windows asks before its first launch (csrc/host/inflate_sample.cc: bgzf_last_byte) through
    tools/bgzf_text_ends_check.cc built with ASan + UBSan: texts with and without their last newline, the last member stored,
    of one byte, and with EOF members behind it"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = tmp_path / "bgzf_text_ends_check"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([cxx] + flags + extra + ["-o", str(exe), os.path.join(root, "tools", "bgzf_text_ends_check.cc")], capture_output=True, text=True)
        if p.returncode == 0 and subprocess.run([str(exe)], capture_output=True).returncode == 2:  # (its usage line)
            break
    else:
        pytest.skip("%s has no sanitizer runtime here: %s" % (cxx, p.stderr.strip()[-200:]))
    records = []
    for _, _, text, _ in texts[::2]:
        text = text[:3 * W]
        for t in (text[:text.rindex(b"\n") + 1], text[:text.rindex(b"\n")]):
            n = len(t)
            records.append((stream_of(t, [W, W, n - 2 * W], "level6"), t, False))
            records.append((stream_of(t, [W, W, n - 2 * W - 1, 1], ["level1", "level1", "level1", "stored"]), t, False))
            records.append((stream_of(t, [W, 0, 0, W, n - 2 * W, 0, 0], "level1", eof=False), t, False))
    path = tmp_path / "cases.bin"
    write_check_file(str(path), records)
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert p.returncode == 0 and "%d records: %d answered" % (len(records), len(records)) in p.stdout, (p.stdout + p.stderr)[-2000:]
