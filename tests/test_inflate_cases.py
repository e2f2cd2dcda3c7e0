"""The inflate decoder's text (csrc/inflate_block.h) and the member walk (csrc/bgzf_walk.h) on the host, pinned to Python's
zlib: host.bgzf_decode_host, and the same text in a program of its own under AddressSanitizer and UBSan.  CPU only."""
import os
import shutil
import subprocess

import pytest

import inflate_cases as ic
from yacrd_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MUTATIONS = 2000


def decode(blob):
    """the text, or None when the decoder refuses"""
    try:
        return host.bgzf_decode_host(blob)
    except host.HostError:
        return None


@pytest.fixture(scope="module")
def valid():
    return ic.valid_cases()


@pytest.fixture(scope="module")
def mutated():
    """[(stream, what zlib says)]"""
    return [(b, ic.zlib_says(b)) for b in ic.mutations(N_MUTATIONS)]


def test_the_symbol_is_exported():
    assert "yacrd_bgzf_decode_host" in host.EXPORTED_SYMBOLS
    assert callable(host.bgzf_decode_host)


def test_valid_streams_give_their_text(valid):
    for name, blob, text in valid:
        assert ic.zlib_says(blob) == text, name  # (the case is what it says)
        assert host.bgzf_decode_host(blob) == text, name


def test_the_encoders_streams_give_their_text():
    for name, blob, text in ic.encoder_cases(range(200)):
        assert host.bgzf_decode_host(blob) == text, name


def test_members_not_taken_name_their_cause():
    for name, blob, cause in ic.not_taken_cases():
        with pytest.raises(host.HostError) as e:
            host.bgzf_decode_host(blob)
        assert "not taken" in str(e.value) and cause in str(e.value), (name, str(e.value))


def test_framings_that_are_not_bgzf():
    for name, blob in ic.not_bgzf_cases():
        with pytest.raises(host.HostError) as e:
            host.bgzf_decode_host(blob)
        assert "not BGZF" in str(e.value), (name, str(e.value))


def test_mutations_are_refused_or_zlibs_bytes(mutated):
    """every one of the seeded mutations, case by case: a refusal, or exactly what zlib returns with CRC and ISIZE matching"""
    taken = refused = 0
    for k, (blob, want) in enumerate(mutated):
        got = decode(blob)
        if got is None:
            refused += 1
            continue
        taken += 1
        assert want is not None, "mutation %d: taken, but zlib does not take it" % k
        assert got == want, "mutation %d: bytes differ from zlib's" % k
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
    exe = tmp_path / "inflate_check"
    subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tools", "inflate_check.cc")], check=True)
    return str(exe), None


def test_the_same_inputs_under_the_sanitizers(tmp_path, valid, mutated):
    """tools/inflate_check.cc: the decoder's text in a program of its own, built with -fsanitize=address,undefined, over the
    valid, not-taken and mutated inputs; every stream in an allocation of exactly its size"""
    exe, why = _sanitizer_build(tmp_path)
    if exe is None:
        pytest.skip(why)
    records = [(b, t, False) for _, b, t in valid] + [(b, t, False) for _, b, t in ic.encoder_cases(range(0, 200, 10))]
    records += [(b, None, False) for _, b, _ in ic.not_taken_cases()] + [(b, None, False) for _, b in ic.not_bgzf_cases()]
    records += [(b, want, True) for b, want in mutated]
    path = tmp_path / "cases.bin"
    ic.write_check_file(str(path), records)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "%d records" % len(records) in p.stdout and " 0 not as expected" in p.stdout, p.stdout
