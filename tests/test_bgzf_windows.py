"""Where the windows of a BGZF text end (csrc/bgzf_windows.h): host.bgzf_window_cuts against the rule restated in Python
(tests/edit_bgzf_window_cases.py: member_cuts) on seeded member sets, the rule's properties, the cuts at the caps' edges, and
the same cases through tools/bgzf_windows_check.cc under AddressSanitizer and UBSan.  CPU only."""
import os
import shutil
import struct
import subprocess

import pytest

from deflate_cases import EOF_MEMBER
from edit_bgzf_window_cases import (W_BGZF, check_cut_properties, cuts_of, frames_of, member_cuts, seeded_member_sets, stream_of,
                                    synthetic_stream)
from yacrd_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = W_BGZF


def specific_cases():
    """[(name, stream, W, the (m0, m1) of every window)]"""
    out = []

    def syn(name, members, want, w=W):
        out.append((name, synthetic_stream([m[0] for m in members], [m[1] for m in members]), w, want))

    syn("the text cap exact: a window of exactly W bytes of text", [(32768, 900), (32768, 900), (100, 60)], [(0, 2), (2, 3)])
    syn("one byte over the text cap", [(32768, 900), (32769, 900), (100, 60)], [(0, 1), (1, 3)])
    syn("the compressed cap exact", [(10, 32768), (10, 32768), (10, 26)], [(0, 2), (2, 3)])
    syn("one byte over the compressed cap", [(10, 32768), (10, 32769), (10, 26)], [(0, 1), (1, 3)])
    two = stream_of(b"A" * 65520, [32760, 32760], "stored")
    assert frames_of(two)[1] == [32791, 32791, 28]  # (65 520 bytes of text fit a window, 65 582 bytes of frames do not)
    out.append(("the compressed cap binding: two stored members of 32 760 bytes", two, W, [(0, 1), (1, 3)]))
    full = (65536, 65536)
    per = W // 28
    syn("3 000 EOF members in a row: windows with no text", [full] + [(0, 28)] * 3000 + [full],
        [(0, 1), (1, 1 + per), (1 + per, 3001), (3001, 3002)])
    syn("trailing EOF members in a window of their own", [(100, 60), full, (0, 28), (0, 28)], [(0, 1), (1, 2), (2, 4)])
    syn("a single member", [(65536, 65536)], [(0, 1)])
    syn("a single EOF member", [(0, 28)], [(0, 1)])
    syn("EOF members alone, more than a window of them", [(0, 28)] * (per + 5), [(0, per), (per, per + 5)])
    syn("no members", [], [])
    syn("a larger window: neither cap binds", [(65536, 30000)] * 10, [(0, 10)], w=1 << 20)
    syn("a larger window, not a multiple of anything", [(65536, 30000)] * 10, [(0, 3), (3, 6), (6, 9), (9, 10)], w=200000)
    return out


@pytest.fixture(scope="module")
def sets():
    return seeded_member_sets()


def _host_cuts(blob, w):
    cuts = host.bgzf_window_cuts(blob, w)
    isizes, frames = frames_of(blob)
    assert cuts == member_cuts(isizes, frames, w)
    check_cut_properties(cuts, isizes, frames, w)
    return cuts


def test_the_symbol_is_exported():
    assert "yacrd_bgzf_window_cuts" in host.EXPORTED_SYMBOLS and callable(host.bgzf_window_cuts)


def test_seeded_member_sets(sets):
    n = 0
    for isizes, frames in sets:
        blob = synthetic_stream(isizes, frames)
        assert frames_of(blob) == (isizes, frames)
        for w in (W, W + 1, 100000, 1 << 20, 1 << 27):
            n += len(_host_cuts(blob, w))
    assert n > 2000


def test_specific_cuts():
    for name, blob, w, want in specific_cases():
        cuts = _host_cuts(blob, w)
        assert [(c[0], c[1]) for c in cuts] == want, name
    name, blob, w, _ = specific_cases()[0]
    assert _host_cuts(blob, w)[0][4:] == (0, W), name
    eofs = [c for c in _host_cuts(specific_cases()[5][1], W) if c[5] == c[4]]
    assert len(eofs) == 2  # (two windows that hold no text at all)


def test_real_streams_cut_as_their_frames_say():
    text = bytes(range(256)) * 1200
    for kind in ("stored", "level1", "level6"):
        blob = stream_of(text, [60000] * 5 + [7200], kind)
        assert sum(frames_of(blob)[0]) == len(text)
        assert _host_cuts(blob, W) == cuts_of(blob, W) and len(_host_cuts(blob, W)) >= 5


def test_what_is_refused():
    for w in (0, 1, 32768, 65535):
        with pytest.raises(host.HostError, match="65 536"):
            host.bgzf_window_cuts(EOF_MEMBER, w)
    with pytest.raises(host.HostError, match="not BGZF"):
        host.bgzf_window_cuts(b"\x1f\x8b\x08\x00" + b"\0" * 20, W)


def write_cuts_file(path, records):
    """records: (stream, W, windows expected) -> the file tools/bgzf_windows_check.cc reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(records)))
        for blob, w, want in records:
            f.write(struct.pack("<QQQ", len(blob), w, want))
            f.write(blob)


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
    exe = tmp_path / "bgzf_windows_check"
    subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tools", "bgzf_windows_check.cc")], check=True)
    return str(exe), None


def test_the_same_cases_under_the_sanitizers(tmp_path, sets):
    """tools/bgzf_windows_check.cc: the rule in a program of its own, built with -fsanitize=address,undefined, over the same
    member sets and the specific cuts; stream and member table each in an allocation of exactly its size"""
    exe, why = _sanitizer_build(tmp_path)
    if exe is None:
        pytest.skip(why)
    records = []
    for isizes, frames in sets:
        blob = synthetic_stream(isizes, frames)
        for w in (W, W + 1, 100000, 1 << 20):
            records.append((blob, w, len(member_cuts(isizes, frames, w))))
    for _, blob, w, want in specific_cases():
        records.append((blob, w, len(want)))
    records.append((EOF_MEMBER, 65535, 0))  # (refused)
    path = tmp_path / "cases.bin"
    write_cuts_file(str(path), records)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "%d records" % len(records) in p.stdout and " 0 not as expected" in p.stdout, p.stdout
