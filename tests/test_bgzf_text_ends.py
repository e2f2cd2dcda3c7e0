"""What the device overlap editor asks of a BGZF text before its first launch (csrc/host/inflate_sample.cc: bgzf_text_ends,
exported as yacrd_bgzf_text_ends): the field count of the first non-empty line and whether the text ends in a newline, from
the first members and the last one alone.  host.bgzf_text_ends against the plain rule restated here in Python, and the
same streams through tools/bgzf_text_ends_check.cc under AddressSanitizer and UBSan.  CPU only."""
import os
import random
import shutil
import subprocess

import pytest

import inflate_cases as ic
from deflate_cases import EOF_MEMBER, paf_like
from yacrd_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = 1 << 20


def plain_rule(text, delim):
    """gpu_edit.hip's first_line_fields: (fields of the first non-empty line, 0 when there is none; last byte is '\\n')"""
    ends_nl = text == b"" or text.endswith(b"\n")
    for line in text.split(b"\n"):
        if line != b"":
            return line.count(delim) + 1, ends_nl
    return 0, ends_nl


def texts():
    r = random.Random(4242)
    paf = paf_like(r, 40)
    m4 = b"".join(b"r%d r%d 0.1 2 0 10 900 1000 0 20 880 1000\n" % (k, k + 1) for k in range(50))
    return [
        ("PAF", paf),
        ("M4", m4),
        ("PAF, the last line without its newline", paf[:-1]),
        ("M4, the last line without its newline", m4[:-1]),
        ("leading empty lines", b"\n" * 300 + paf),
        ("empty lines only", b"\n" * 50),
        ("one line, no newline", b"a\tb c\td"),
        ("one byte", b"x"),
        ("one newline", b"\n"),
        ("a line of a CR", b"\r\n" + paf),
        ("a quote in the first line", b'a\t"b\tc"\td\n'),
        ("delimiters only", b"\t\t  \t\n"),
        ("empty", b""),
    ]


def streams():
    """[(name, stream, text or None: must be refused)]"""
    out = []
    for name, text in texts():
        for chunk in (1, 7, 100, 65280):
            if chunk == 1 and len(text) > 600:
                continue  # (a member per byte of a few hundred bytes shows what a member per byte of thousands does)
            out.append(("%s, chunk %d" % (name, chunk), ic.bgzf_of(text, chunk), text))
    r = random.Random(77)
    paf = paf_like(r, 30)
    first = paf.split(b"\n")[0] + b"\n"
    a, b = len(first) // 3, 2 * len(first) // 3
    out.append(("the first line crosses three members", ic.member(first[:a]) + ic.member(first[a:b]) + ic.member(first[b:] + paf) + EOF_MEMBER,
                first + paf))
    out.append(("the first non-empty line starts in the third member", ic.member(b"\n\n") + ic.member(b"\n") + ic.member(paf) + EOF_MEMBER, b"\n\n\n" + paf))
    out.append(("a last data member of one byte, the newline", ic.member(paf[:-1]) + ic.member(b"\n") + EOF_MEMBER, paf))
    out.append(("a last data member of one byte, no newline", ic.member(paf) + ic.member(b"x") + EOF_MEMBER, paf + b"x"))
    out.append(("EOF members in the middle and at the end", EOF_MEMBER + ic.member(paf[:100]) + EOF_MEMBER + EOF_MEMBER + ic.member(paf[100:]) +
                EOF_MEMBER + EOF_MEMBER, paf))
    out.append(("no EOF member", ic.member(paf[:100]) + ic.member(paf[100:-1]), paf[:-1]))
    out.append(("an empty stream", b"", b""))
    out.append(("EOF members only", EOF_MEMBER * 3, b""))
    # the sample: a first line that ends exactly with it, one byte beyond it, and far beyond it
    line = (b"id\t" + b"ACGT" * (SAMPLE // 4))[:SAMPLE - 1] + b"\n"
    out.append(("a first line that fills the sample", ic.bgzf_of(line + b"a\tb\n", 65536, level=1), line + b"a\tb\n"))
    out.append(("a first line one byte longer than the sample", ic.bgzf_of(b"x" + line + b"a\tb\n", 65536, level=1), None))
    out.append(("a first line of the whole text, longer than the sample", ic.bgzf_of(b"xy" + line[:-1], 65536, level=1), None))
    out.append(("empty lines beyond the sample", ic.bgzf_of(b"\n" * (SAMPLE + 5) + b"a\tb\n", 65536, level=1), None))
    # members the decoder does not take, where the helper looks: the first, the last
    good, dead = ic.member(paf), ic.frame(ic.deflate(paf), paf, crc=1)
    out.append(("a damaged first member", dead + good + EOF_MEMBER, None))
    out.append(("a damaged last member", good + dead + EOF_MEMBER, None))
    out.append(("a damaged member where the first line ends", ic.member(b"a\tb") + ic.frame(ic.deflate(b"\tc\n"), b"\tc\n", crc=2) + good + EOF_MEMBER, None))
    for name, blob, _ in ic.not_taken_cases()[:-1]:
        out.append(("first member: " + name, blob[:-len(EOF_MEMBER)] + good + EOF_MEMBER, None))
    for name, blob in ic.not_bgzf_cases():
        out.append(("not BGZF: " + name, blob, None))
    return out


@pytest.fixture(scope="module")
def cases():
    return streams()


def test_the_symbol_is_exported():
    assert "yacrd_bgzf_text_ends" in host.EXPORTED_SYMBOLS
    assert callable(host.bgzf_text_ends)


def test_every_stream_against_the_plain_rule(cases):
    n_answered = n_refused = 0
    for name, blob, text in cases:
        for delim in (b"\t", b" "):
            if text is None:
                with pytest.raises(host.HostError):
                    host.bgzf_text_ends(blob, delim)
                n_refused += 1
            else:
                assert ic.zlib_says(blob) == text, name
                assert host.bgzf_text_ends(blob, delim) == plain_rule(text, delim), name
                n_answered += 1
    assert n_answered > 80 and n_refused > 40


def test_the_message_names_the_cause():
    good = ic.member(b"a\tb\n")
    for name, blob, cause in ic.not_taken_cases()[:-1]:
        with pytest.raises(host.HostError, match="does not take") as ei:
            host.bgzf_text_ends(blob[:-len(EOF_MEMBER)] + good + EOF_MEMBER, b"\t")
        assert cause in str(ei.value), name
    with pytest.raises(host.HostError, match="not BGZF"):
        host.bgzf_text_ends(ic.not_bgzf_cases()[0][1], b"\t")
    with pytest.raises(host.HostError, match="not complete"):
        host.bgzf_text_ends(ic.bgzf_of(b"x" * (SAMPLE + 1) + b"\n", 65536, level=1), b"\t")


def test_a_damaged_member_behind_the_first_line_is_the_devices_to_refuse():
    """the helper decodes no further than the first line's end, and the last member: what lies between is not its business"""
    good = ic.member(b"a\tb\n")
    blob = good + ic.frame(ic.deflate(b"c\td\n"), b"c\td\n", crc=1) + good + EOF_MEMBER
    assert host.bgzf_text_ends(blob, b"\t") == (2, True)


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
    exe = tmp_path / "bgzf_text_ends_check"
    subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tools", "bgzf_text_ends_check.cc")], check=True)
    return str(exe), None


def test_the_same_streams_under_the_sanitizers(tmp_path, cases):
    """tools/bgzf_text_ends_check.cc: the helper in a program of its own, built with -fsanitize=address,undefined, over the
    same streams; stream and member table each in an allocation of exactly its size"""
    exe, why = _sanitizer_build(tmp_path)
    if exe is None:
        pytest.skip(why)
    records = [(blob, text, False) for _, blob, text in cases]
    path = tmp_path / "cases.bin"
    ic.write_check_file(str(path), records)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "%d records" % len(records) in p.stdout and " 0 not as expected" in p.stdout, p.stdout
