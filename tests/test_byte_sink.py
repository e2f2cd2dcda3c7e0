"""yacrd_edit_file_to (the edited bytes to a sink instead of a file), yacrd_file_compression, and the device deflate
encoder's text compiled for the host: its code lengths, and its BGZF bytes against zlib.  CPU only."""
import bz2
import gzip
import lzma
import os
import random
import shutil
import zlib

import numpy as np
import pytest

import oracle
from yacrd_amd import host

from deflate_cases import BLOCK, EOF_MEMBER, fastq_like, fuzz_text, huffman_only_size, paf_like, walk_bgzf

OPS = {"scrubb": host.OP_SCRUBB, "filter": host.OP_FILTER, "extract": host.OP_EXTRACT, "split": host.OP_SPLIT}


@pytest.fixture(scope="module")
def table(golden_dir):
    with open(os.path.join(golden_dir, "reads.paf")) as f:
        names, offsets, intervals, lengths = oracle.to_csr(oracle.parse_paf(f))
    bo, br, rt = oracle.run(offsets, intervals, lengths, 0, 0.8)
    return names, lengths.astype(np.uint32), bo, br, rt


@pytest.fixture(scope="module")
def inputs(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("sink")
    gz = os.path.join(golden_dir, "reads.fastq.gz")
    shutil.copy(gz, d / "reads.fastq.gz")
    text = gzip.open(gz, "rb").read()
    (d / "reads.fastq").write_bytes(text)
    # the same reads as FASTA, the sequence folded to 60 columns
    recs = text.split(b"\n")
    fa = []
    for i in range(0, len(recs) - 3, 4):
        seq = recs[i + 1]
        fa.append(b">" + recs[i][1:] + b"\n" + b"\n".join(seq[k:k + 60] for k in range(0, len(seq), 60)) + b"\n")
    (d / "reads.fasta").write_bytes(b"".join(fa))
    shutil.copy(os.path.join(golden_dir, "reads.paf"), d / "reads.paf")
    return d


def collect(op, path, table, n_threads):
    got = []
    host.edit_file_to(OPS[op], str(path), lambda b: got.append(b) and None, *table, n_threads=n_threads)
    return b"".join(got)


@pytest.mark.parametrize("n_threads", [1, 4])
@pytest.mark.parametrize("op", ["scrubb", "filter", "extract", "split"])
@pytest.mark.parametrize("name", ["reads.fastq", "reads.fastq.gz", "reads.fasta"])
def test_sink_gets_the_files_bytes(inputs, table, tmp_path, name, op, n_threads):
    plain = inputs / name.replace(".gz", "")
    out = tmp_path / ("out." + name.replace(".gz", ""))
    host.edit_file(OPS[op], str(plain), str(out), *table)
    assert collect(op, inputs / name, table, n_threads) == out.read_bytes()


@pytest.mark.parametrize("op", ["scrubb", "filter", "extract", "split"])
def test_sink_gets_the_truth(inputs, table, golden_dir, op):
    truth = gzip.open(os.path.join(golden_dir, "truth.%s.fastq.gz" % op), "rb").read()
    assert collect(op, inputs / "reads.fastq.gz", table, 1) == truth


@pytest.mark.parametrize("n_threads", [1, 4])
@pytest.mark.parametrize("op", ["filter", "extract"])
def test_sink_overlaps(inputs, table, tmp_path, op, n_threads):
    out = tmp_path / "out.paf"
    host.edit_file(OPS[op], str(inputs / "reads.paf"), str(out), *table)
    assert collect(op, inputs / "reads.paf", table, n_threads) == out.read_bytes()
    assert out.stat().st_size > 0


def test_sink_that_refuses(inputs, table):
    calls = []

    def sink(b):
        calls.append(len(b))
        return sum(calls) >= 100000  # (stop once this many bytes have arrived)
    with pytest.raises(host.HostError):
        host.edit_file_to(host.OP_SCRUBB, str(inputs / "reads.fastq"), sink, *table)
    assert sum(calls) >= 100000 and sum(calls[:-1]) < 100000, "nothing arrives after the refusal"


def test_sink_that_raises(inputs, table):
    def sink(b):
        raise KeyError("from the sink")
    with pytest.raises(KeyError):
        host.edit_file_to(host.OP_SCRUBB, str(inputs / "reads.fastq"), sink, *table)


def test_sink_bad_operation(inputs, table):
    with pytest.raises(host.HostError):
        host.edit_file_to(host.OP_SCRUBB, str(inputs / "reads.paf"), lambda b: None, *table)


def test_file_compression(tmp_path):
    data = b"@r\nACGT\n+\n????\n" * 9000
    (tmp_path / "plain").write_bytes(data)
    (tmp_path / "gz").write_bytes(gzip.compress(data))
    (tmp_path / "bgzf").write_bytes(host.bgzf_encode_host(data))
    (tmp_path / "bz2").write_bytes(bz2.compress(data))
    (tmp_path / "xz").write_bytes(lzma.compress(data))
    (tmp_path / "empty").write_bytes(b"")
    got = [host.file_compression(str(tmp_path / n)) for n in ("plain", "gz", "bgzf", "bz2", "xz", "empty", "missing")]
    assert got == [0, 1, 1, 2, 3, 0, 0]


# ---- the encoder's code lengths ---------------------------------------------------------------------------------------
def kraft(lens):
    return sum(2.0 ** -int(l) for l in lens if l)


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def huffman_cost(weights):
    import heapq
    h, cost = list(weights), 0
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


@pytest.mark.parametrize("limit", [7, 15])
def test_code_lengths(limit):
    n_max = 19 if limit == 7 else 286
    cases = [fib(min(n_max, 40)), [1] * n_max, [0] * (n_max - 1) + [5], [7, 0, 3] + [0] * (n_max - 3), [65280] + [1] * (n_max - 1),
             [2 ** min(i, 30) for i in range(n_max)]]
    r = random.Random(3)
    cases += [[r.choice([0, 0, 1, 2, 50, 4000, 60000]) for _ in range(n_max)] for _ in range(50)]
    cases += [[r.choice([0, 0, 0, 0, 0, 1, 1, 2, 3, 9]) for _ in range(n_max)] for _ in range(200)]
    for freq in cases:
        freq = freq + [0] * (n_max - len(freq))
        lens = host.deflate_code_lengths(freq, limit)
        assert lens.max() <= limit
        assert all(l > 0 for l, f in zip(lens, freq) if f), "every used symbol has a code"
        assert kraft(lens) == 1.0, "the code is complete"
        used = [f for f in freq if f]
        # a Huffman tree of depth d weighs at least fib(d + 2): below that no tie-breaking needs the limit, and the cost is the optimum
        if len(used) >= 2 and sum(used) < fib(limit + 3)[-1]:
            assert sum(f * int(l) for f, l in zip(freq, lens)) == huffman_cost(used)


# ---- the encoder's bytes, one host thread playing the workgroup -------------------------------------------------------
def check(data):
    blob = host.bgzf_encode_host(data)
    assert gzip.decompress(blob) == data
    members = walk_bgzf(blob)
    assert members[-1][0] == EOF_MEMBER and len(members) - 1 == (len(data) + BLOCK - 1) // BLOCK
    assert b"".join(d for _, d in members) == data
    assert all(len(d) == BLOCK for _, d in members[:-2])
    if len(data) >= BLOCK:
        assert len(blob) <= 1.02 * huffman_only_size(data) + 28
    assert len(blob) <= len(data) + 31 * (len(members) - 1) + 28
    return blob


def test_host_encoder_edges():
    r = random.Random(5)
    for data in [b"", b"x", r.randbytes(BLOCK - 1), r.randbytes(BLOCK), r.randbytes(BLOCK + 1), r.randbytes(2 * BLOCK + 1), bytes(1 << 20),
                 b"\xff" * (1 << 20), bytes(range(256)) * 600, b"no newline at the end"]:
        check(data)
    for period in list(range(2, 301, 7)) + [255, 256, 257, 258, 259, 300]:
        check((r.randbytes(period) * (150000 // period + 1))[:150000])


def test_host_encoder_finds_matches(golden_dir):
    r = random.Random(6)
    for data in [open(os.path.join(golden_dir, "reads.paf"), "rb").read(), fastq_like(r, 900, const_quality=True), bytes(1 << 20), paf_like(r, 3000)]:
        assert len(check(data)) < huffman_only_size(data)


def test_host_encoder_golden_fastq(golden_dir):
    data = gzip.open(os.path.join(golden_dir, "reads.fastq.gz"), "rb").read()
    blob = check(data)
    assert len(blob) < huffman_only_size(data)


def test_host_encoder_fuzz():
    for seed in range(300):
        check(fuzz_text(seed))
