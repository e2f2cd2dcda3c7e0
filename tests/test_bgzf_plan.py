"""The planner of the segment-wise device inflate (csrc/bgzf_plan.h): which members to launch and which text segment to
hand on as the compressed bytes land.  host.bgzf_plan_segments over member sets and landing schedules, every property of
the contract asserted here in Python, and the same schedules through tools/bgzf_plan_check.cc under AddressSanitizer and
UBSan.  CPU only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import inflate_cases as ic
from deflate_cases import EOF_MEMBER
from yacrd_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, SEG = 4 << 20, 32  # the mover's


def _tiny(sizes):
    return b"".join(ic.member(bytes([65 + k % 26]) * n) for k, n in enumerate(sizes))


def member_sets():
    """[(name, BGZF stream, small: one byte at a time is affordable)]"""
    out = [(name, blob, len(blob) <= 4096) for name, blob, _ in ic.valid_cases()]
    out.append(("members of 1-7 bytes", _tiny(range(1, 8)) + EOF_MEMBER, True))
    out.append(("members of 1-7 bytes, no EOF member", _tiny(range(1, 8)), True))
    out.append(("EOF members first, in the middle and last", EOF_MEMBER + _tiny([3, 5]) + EOF_MEMBER + EOF_MEMBER + _tiny([7]) + EOF_MEMBER, True))
    out.append(("EOF members only", EOF_MEMBER * 3, True))
    out.append(("zero members", b"", True))
    out.append(("1 031 members", _tiny([1 + k % 7 for k in range(1031)]) + EOF_MEMBER, False))
    return out


def _next_end(blob, at):
    # (an empty payload: the member's size from its BC subfield)
    h = blob[at:]
    end = 12 + struct.unpack("<H", h[10:12])[0]
    q = 12
    while q + 4 <= end:
        slen = struct.unpack("<H", h[q + 2:q + 4])[0]
        if h[q:q + 2] == b"BC":
            return at + struct.unpack("<H", h[q + 4:q + 6])[0] + 1
        q += 4 + slen
    raise AssertionError("no BC subfield")


def member_ends(blob):
    """the same from the BC subfields alone: members tile the stream"""
    ends, at = [], 0
    while at < len(blob):
        at = _next_end(blob, at)
        ends.append(at)
    return ends


_CACHE = {}


def _ends_of(blob):
    if blob not in _CACHE:
        _CACHE[blob] = (member_ends(blob), [isize for _, _, isize in ic.walk(blob)])
    return _CACHE[blob][0]


def _isizes_of(blob):
    _ends_of(blob)
    return _CACHE[blob][1]


def schedules(blob, small):
    """[(name, landed compressed bytes, call after call)]: the last entry is always the stream's size"""
    n = len(blob)
    out = [("everything at once", [n]), ("4 MiB chunks", list(range(CHUNK, n, CHUNK)) + [n]), ("the same landing twice", [n // 2, n // 2, n, n])]
    if small:
        out.append(("one byte at a time", list(range(0, n + 1))))
    ends = _ends_of(blob)
    edge = sorted(set(x for e in ends[:40] + ends[-3:] for x in (e - 1, e)))
    out.append(("on every trailer's last byte, and one short of it", [x for x in edge if 0 <= x <= n] + [n]))
    for k, e in enumerate(ends[:3]):
        out.append(("one byte short of member %d, then the rest" % k, [e - 1, n]))
        out.append(("exactly member %d, then the rest" % k, [e, n]))
    return out


def units(blob):
    """(chunk, seg_chunks) to plan with: the mover's, and small ones that cut these small texts into many segments"""
    if sum(_isizes_of(blob)) > 8192:  # (a step per byte of a large text proves nothing more, slowly)
        return [(CHUNK, SEG), (1000, 3), (4096, 32)]
    return [(CHUNK, SEG), (1, 1), (4, 3), (64, 2), (4096, 32)]


def check(blob, landed, chunk, seg):
    """the four properties; returns the steps"""
    members, steps = host.bgzf_plan_segments(blob, landed, chunk, seg)
    in_off, csize, isize, out_off = (members[:, k].tolist() for k in range(4))
    M, n = len(members), sum(isize)
    done = [o + c + 8 for o, c in zip(in_off, csize)]  # a member is complete when this many bytes have landed
    assert done == _ends_of(blob) and isize == _isizes_of(blob)
    next_m = next_t = 0
    for row in steps.tolist():
        call, m0, m1, inflated, t0, t1, avail, last = row
        have = int(landed[call])
        # 1. every member exactly once, only when complete (and none that is complete is left behind)
        assert m0 == next_m and m0 <= m1 <= M
        assert all(done[m] <= have for m in range(m0, m1))
        assert m1 == M or done[m1] > have
        next_m = m1
        # 2. what is inflated: the first unlaunched member's place, or all of it
        assert inflated == (out_off[m1] if m1 < M else n)
        # 3. the text segments: in order, on chunk boundaries, a whole segment or the last; avail within the inflated text
        if t1 > t0:
            assert t0 == next_t and t0 % chunk == 0 and t1 % chunk == 0
            assert t1 - t0 == seg * chunk or t1 >= n
            assert t1 - t0 <= seg * chunk and t0 < n
            assert avail <= inflated and avail <= n
            assert avail == n or avail >= t1 + chunk
            next_t = t1
        else:
            assert t0 == t1
        assert (last == 1) == (next_m == M and next_t >= n)
    assert next_m == M, "members never launched"
    assert next_t >= n, "text never handed on"
    assert next_t < n + chunk
    # 4. one step ends the text, and it is the last one
    assert len(steps) >= 1 and int(steps[-1][7]) == 1 and int(steps[:, 7].sum()) == 1
    return steps


@pytest.fixture(scope="module")
def sets():
    return member_sets()


def test_the_symbol_is_exported():
    assert "yacrd_bgzf_plan_segments" in host.EXPORTED_SYMBOLS
    assert callable(host.bgzf_plan_segments)


def test_every_set_under_every_schedule(sets):
    n_checked = 0
    for name, blob, small in sets:
        for sname, landed in schedules(blob, small):
            for chunk, seg in units(blob):
                if len(landed) > 4096 and chunk not in (CHUNK, 4):
                    continue  # (the long schedules with two units only)
                try:
                    check(blob, landed, chunk, seg)
                except AssertionError as e:
                    raise AssertionError("%s / %s / chunk %d x %d: %s" % (name, sname, chunk, seg, e))
                n_checked += 1
    assert n_checked > 400


def test_a_text_of_no_bytes_is_one_empty_step(sets):
    for blob, n_members in ((b"", 0), (EOF_MEMBER, 1), (EOF_MEMBER * 3, 3)):
        steps = check(blob, [len(blob)], CHUNK, SEG)
        assert steps.tolist() == [[0, 0, n_members, 0, 0, 0, 0, 1]]
    # one byte at a time: the EOF members as they complete, the text ends with the last of them, no segment anywhere
    steps = check(EOF_MEMBER * 3, list(range(3 * len(EOF_MEMBER) + 1)), CHUNK, SEG)
    assert [int(r[2]) for r in steps] == [1, 2, 3] and all(int(r[4]) == int(r[5]) == 0 for r in steps)


def test_a_member_launches_on_its_last_trailer_byte_and_not_one_short(sets):
    for name, blob, _ in sets:
        ends = member_ends(blob)
        for k, e in enumerate(ends[:5]):
            _, short = host.bgzf_plan_segments(blob, [e - 1])
            _, exact = host.bgzf_plan_segments(blob, [e])
            assert sum(int(r[2]) - int(r[1]) for r in short) == k, name
            assert sum(int(r[2]) - int(r[1]) for r in exact) == k + 1, name


def test_segments_at_the_movers_unit():
    """a text over one segment from members whose compressed stream is far under one: the layout the level-1 GPU case has,
    here from stored 1-byte members planned with a 1-byte chunk (the arithmetic is the same at 4 MiB)"""
    blob = _tiny([1] * 100) + EOF_MEMBER
    ends = member_ends(blob)
    steps = check(blob, [ends[39], ends[69], len(blob)], 1, 32)
    segs = [(int(r[4]), int(r[5]), int(r[6])) for r in steps if int(r[5]) > int(r[4])]
    assert segs == [(0, 32, 33), (32, 64, 65), (64, 96, 97), (96, 100, 100)]
    assert [int(r[0]) for r in steps if int(r[5]) > int(r[4])] == [0, 1, 2, 2]


def test_what_is_refused():
    with pytest.raises(host.HostError):
        host.bgzf_plan_segments(b"\x1f\x8b\x08\x00" + b"\0" * 20, [24])
    with pytest.raises(host.HostError):
        host.bgzf_plan_segments(EOF_MEMBER, [5, 4])


def write_plan_file(path, records):
    """records: (stream, chunk, seg_chunks, landed) -> the file tools/bgzf_plan_check.cc reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(records)))
        for blob, chunk, seg, landed in records:
            f.write(struct.pack("<QQQQ", len(blob), chunk, seg, len(landed)))
            f.write(blob)
            f.write(np.asarray(landed, dtype="<u8").tobytes())


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
    exe = tmp_path / "bgzf_plan_check"
    subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "tools", "bgzf_plan_check.cc")], check=True)
    return str(exe), None


def test_the_same_schedules_under_the_sanitizers(tmp_path, sets):
    """tools/bgzf_plan_check.cc: the planner in a program of its own, built with -fsanitize=address,undefined, over the same
    member sets and schedules; stream, schedule and member table each in an allocation of exactly its size"""
    exe, why = _sanitizer_build(tmp_path)
    if exe is None:
        pytest.skip(why)
    records = []
    for _, blob, small in sets:
        for _, landed in schedules(blob, small):
            for chunk, seg in units(blob):
                if len(landed) > 4096 and chunk not in (CHUNK, 4):
                    continue
                records.append((blob, chunk, seg, landed))
    path = tmp_path / "schedules.bin"
    write_plan_file(str(path), records)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "%d records" % len(records) in p.stdout and " 0 not as expected" in p.stdout, p.stdout
