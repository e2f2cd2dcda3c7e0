"""The plain-gzip decoder's text (csrc/inflate_stream.h) and the header walk (csrc/gzip_walk.h) on the host, pinned to
Python's zlib: host.gzip_stream_decode_host at three chunk sizes, the finder's completeness against a pure-Python block
walker, and the same text in a program of its own under AddressSanitizer and UBSan.  CPU only."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import gunzip_stream_cases as gc
from yacrd_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MUTATIONS = 2000
WORKERS = max(1, min(8, os.cpu_count() or 1))


def decode(blob, chunk):
    """the text, or None when the decoder refuses"""
    try:
        return host.gzip_stream_decode_host(blob, chunk)[0]
    except host.HostError:
        return None


@pytest.fixture(scope="module")
def valid():
    return gc.valid_cases()


@pytest.fixture(scope="module")
def mutated():
    """[(stream, chunk, what zlib says)]"""
    return [(b, gc.CHUNKS[k % 3], gc.zlib_says(b)) for k, b in enumerate(gc.mutations(N_MUTATIONS))]


def test_the_symbol_is_exported():
    assert "yacrd_gzip_stream_decode_host" in host.EXPORTED_SYMBOLS
    assert callable(host.gzip_stream_decode_host)


def test_valid_streams_give_zlibs_bytes_at_every_chunk_size(valid):
    for name, blob, text in valid:
        assert gc.zlib_says(blob) == text, name  # (the case is what it says)
        for chunk in gc.CHUNKS:
            got, counters = host.gzip_stream_decode_host(blob, chunk)
            assert got == text, (name, chunk)
            assert counters["out_bytes"] == len(text) and counters["n_chunks"] == max(1, -(-len(gc.payload_of(blob)) // chunk)), (name, chunk)
    assert host.gzip_stream_decode_host(valid[0][1])[0] == valid[0][2]  # (the default chunk)


def test_the_finder_misses_no_dynamic_block_start(valid):
    """n_spans >= 1 + the chunks k >= 1 that hold a dynamic non-final block start by the Python walker: a decoder that fell
    back to one span would give the right bytes and must not pass.  The floors are the counts the streams were made for."""
    spans = {}
    for name, blob, _ in valid:
        for chunk in gc.CHUNKS:
            counters = host.gzip_stream_decode_host(blob, chunk)[1]
            need = 1 + gc.chunks_with_a_start(blob, chunk)
            assert counters["n_spans"] >= need, (name, chunk, counters, need)
            spans[name, chunk] = counters["n_spans"]
    for lv in (1, 6, 9):
        for what in ("overlaps", "reads"):
            n = [spans["%s, level %d" % (what, lv), c] for c in gc.CHUNKS]
            assert 8 <= n[0] <= 11 and 8 <= n[1] <= 11 and 7 <= n[2] <= 9, (what, lv, n)
    for mode in ("Z_BLOCK", "Z_SYNC_FLUSH"):
        n = [spans["short spans, %s every 3 000 bytes" % mode, c] for c in gc.CHUNKS]
        assert n[0] in (253, 254) and n[1] == 64, (mode, n)


def test_the_walker_counts_what_the_streams_were_made_for(valid):
    by = {name: gc.blocks(gc.payload_of(blob)) for name, blob, _ in valid}
    for lv in (1, 6, 9):
        for what in ("overlaps", "reads"):
            bl = by["%s, level %d" % (what, lv)]
            assert 9 <= len(bl) <= 12 and 3800 <= sum(b[4] for b in bl) <= 18600, (what, lv, len(bl))  # (3 878 .. 18 535 as counted)
    bl = by["short spans, Z_BLOCK every 3 000 bytes"]
    assert sum(1 for b in bl if b[1] == 2 and not b[2]) == 303 and sum(b[4] for b in bl) == 84003
    assert all(b[3] == 3000 for b in bl[:-1])
    bl = by["short spans, Z_SYNC_FLUSH every 3 000 bytes"]
    assert sum(1 for b in bl if b[1] == 2 and not b[2]) == 303 and sum(1 for b in bl if b[1] == 0 and b[3] == 0) == 303


def test_wrong_guesses_cost_rounds_not_bytes(valid):
    by = {name: blob for name, blob, _ in valid}
    got = host.gzip_stream_decode_host(by["a planted false start"], 1024)[1]
    assert got["n_false_starts"] >= 1, got
    got = host.gzip_stream_decode_host(by["a planted false start in front of a real one in its chunk"], 1024)[1]
    assert got["n_false_starts"] >= 1 and got["rounds"] >= 2, got


def test_refused_streams_name_their_cause():
    for name, blob, cause in gc.refused_cases():
        assert gc.zlib_says(blob) is None, name  # (zlib takes none of them as one whole member either)
        for chunk in gc.CHUNKS:
            with pytest.raises(host.HostError) as e:
                host.gzip_stream_decode_host(blob, chunk)
            assert "not taken" in str(e.value) or "not a gzip member" in str(e.value), (name, str(e.value))
            if cause:
                assert cause in str(e.value), (name, str(e.value))


def test_a_span_beyond_the_work_bound_is_refused_not_wrapped():
    """Z_FIXED makes one span of a whole stream: 64 MiB of text is the most one span may make (csrc/inflate_stream.h: kSpanMaxOut)"""
    import zlib
    for n, taken in ((1 << 20, True), ((64 << 20) + 1, False)):
        text = bytes(n)
        blob = gc.gz(gc.deflate(text, 1, zlib.Z_FIXED), text)
        if taken:
            got, counters = host.gzip_stream_decode_host(blob, 32768)
            assert got == text and counters["n_spans"] == 1
        else:
            assert gc.zlib_says(blob) == text  # (a good stream: refused for its size alone)
            with pytest.raises(host.HostError) as e:
                host.gzip_stream_decode_host(blob, 32768)
            assert "a span beyond the decoder's bounds" in str(e.value)


def test_mutations_are_refused_or_zlibs_bytes(mutated):
    """every one of the seeded mutations, case by case: a refusal, or exactly what zlib returns; where zlib refuses, a refusal"""
    with ThreadPoolExecutor(WORKERS) as pool:  # (the library call releases the interpreter's lock)
        got = list(pool.map(lambda m: decode(m[0], m[1]), mutated))
    taken = refused = 0
    for k, ((blob, chunk, want), g) in enumerate(zip(mutated, got)):
        if g is None:
            refused += 1
            continue
        taken += 1
        assert want is not None, "mutation %d: taken, but zlib does not take it" % k
        assert g == want, "mutation %d: bytes differ from zlib's" % k
    assert taken + refused == N_MUTATIONS
    assert taken > 0 and refused > N_MUTATIONS // 2  # (the mutations do both: bits that do not matter, and damage)


def _sanitizer_build(tmp_path):
    """the check program built with ASan + UBSan, or the reason why this machine cannot"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        return None, "no C++ compiler"
    base = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program where the compiler can: the program then does not care what else the process loads
    for flags in (base + ["-static-libasan", "-static-libubsan"], base):
        p = subprocess.run([cxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
        if p.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    else:
        return None, "%s has no sanitizer runtime here: %s" % (cxx, p.stderr.strip()[-200:])
    exe = tmp_path / "inflate_stream_check"
    subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tools", "inflate_stream_check.cc")], check=True)
    return str(exe), None


def test_the_same_inputs_under_the_sanitizers(tmp_path, valid, mutated):
    """tools/inflate_stream_check.cc: the decoder's text and the header walk in a program of their own, built with
    -fsanitize=address,undefined, over the valid (at every chunk size), refused and mutated inputs; every stream in an
    allocation of exactly its size.  The records are dealt to a few files, one process each."""
    exe, why = _sanitizer_build(tmp_path)
    if exe is None:
        pytest.skip(why)
    records = [(b, c, t, False) for _, b, t in valid for c in gc.CHUNKS]
    records += [(b, 1024, None, False) for _, b, _ in gc.refused_cases()]
    records += [(b, c, want, True) for b, c, want in mutated]
    procs = []
    for w in range(WORKERS):
        part = records[w::WORKERS]
        path = tmp_path / ("cases%d.bin" % w)
        gc.write_check_file(str(path), part)
        procs.append((len(part), subprocess.Popen([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for n, p in procs:
        out, err = p.communicate()
        assert p.returncode == 0, (out + err)[-3000:]
        assert "%d records" % n in out and " 0 not as expected" in out, out
