"""What tests/test_bgzf_windows.py, tests/test_edit_bgzf_window_cases.py (CPU) and tests/test_gpu_edit_bgzf_windows.py (GPU)
share: the windows of a BGZF FASTQ / FASTA (csrc/bgzf_windows.h, csrc/gpu_seq_edit.hip: run_windows) restated —
where the windows end, from the members' sizes alone; what every window carries into the next, for windows that end anywhere
—, and builders of BGZF streams whose members have the sizes a case asks for.  The bytes' yardsticks stay
edit_fastq_cases.restate / edit_fasta_cases.restate and the host loop."""
import random
import struct

from deflate_cases import EOF_MEMBER
from inflate_cases import member, stored_member

W_BGZF = 65536  # the smallest window of a BGZF run: the largest frame, the largest ISIZE
ISIZES = (0, 1, 7, 100, 4093, 32768, 65279, 65280, 65536)
KINDS = ("stored", "level1", "level6")


# ---- the cut rule --------------------------------------------------------------------------------------------------------------
def member_cuts(isizes, frame_sizes, W):
    """csrc/bgzf_windows.h restated: greedy — a window takes members while its text and its frames are both at most W bytes,
    and always one.  -> [(m0, m1, c0, c1, t0, t1)]: the members, the stream's bytes that hold their whole frames, the text's"""
    assert W >= W_BGZF and len(isizes) == len(frame_sizes)
    cuts, m, c, t = [], 0, 0, 0
    while m < len(isizes):
        m1, c1, t1 = m, c, t
        while m1 < len(isizes) and (m1 == m or (t1 + isizes[m1] - t <= W and c1 + frame_sizes[m1] - c <= W)):
            c1 += frame_sizes[m1]
            t1 += isizes[m1]
            m1 += 1
        cuts.append((m, m1, c, c1, t, t1))
        m, c, t = m1, c1, t1
    return cuts


def frames_of(blob):
    """(isizes, frame sizes) of a BGZF stream whose members carry BC as their first subfield (every builder's here)"""
    isizes, frames, at = [], [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 14] == b"BC", at
        size = struct.unpack("<H", blob[at + 16:at + 18])[0] + 1
        isizes.append(struct.unpack("<I", blob[at + size - 4:at + size])[0])
        frames.append(size)
        at += size
    return isizes, frames


def cuts_of(blob, W):
    return member_cuts(*frames_of(blob), W)


def check_cut_properties(cuts, isizes, frame_sizes, W):
    """what csrc/bgzf_windows.h promises: the cuts partition [0, M), the stream and the text; both caps hold for every window;
    no window could have taken its successor's first member"""
    M = len(isizes)
    if not M:
        assert cuts == []
        return
    assert cuts[0][0] == 0 and cuts[0][2] == 0 and cuts[0][4] == 0
    assert cuts[-1][1] == M and cuts[-1][3] == sum(frame_sizes) and cuts[-1][5] == sum(isizes)
    for k, (m0, m1, c0, c1, t0, t1) in enumerate(cuts):
        assert m1 > m0 and c1 - c0 == sum(frame_sizes[m0:m1]) and t1 - t0 == sum(isizes[m0:m1])
        assert c1 - c0 <= W and t1 - t0 <= W
        if k:
            assert (m0, c0, t0) == (cuts[k - 1][1], cuts[k - 1][3], cuts[k - 1][5])
        if m1 < M:
            assert t1 - t0 + isizes[m1] > W or c1 - c0 + frame_sizes[m1] > W
    if sum(isizes) <= W and sum(frame_sizes) <= W:
        assert len(cuts) == 1


# ---- the run, window by window, for windows that end anywhere --------------------------------------------------------------------
def _line_ends(win):
    out, at = [], -1
    while True:
        at = win.find(b"\n", at + 1)
        if at < 0:
            return out
        out.append(at)


def window_carries_at(text, borders, fasta, W=None):
    """The run of csrc/gpu_seq_edit.hip: run_windows for windows whose new bytes end at `borders` (rising, not strictly: a
    window may bring no new byte; the last border is len(text)): window k's text is the carry of window k - 1 and then
    text[borders[k - 1]:borders[k]].
    FASTQ: a window completes floor(lines / 4) records and carries what lies behind them; the last must carry nothing.
    FASTA: of a window's whole lines H begin with '>'; a window that is not the last completes max(H - 1, 0) records and
    carries everything from its last header line on — all of it with H = 0 — unless its partial last line begins with '>'
    (H > 0): then all H records are complete and that line alone is carried (the open-header clause).  The last window must
    end with a newline.
    -> the carries of the windows but the last; None when one is longer than W (given) or the last window does not end as
    it must."""
    assert list(borders) == sorted(borders) and borders and borders[-1] == len(text)
    carries, carry, at = [], b"", 0
    for k, b in enumerate(borders):
        win = carry + text[at:b]
        at = b
        last = k + 1 == len(borders)
        ends = _line_ends(win)
        if fasta:
            if last:
                return carries if win.endswith(b"\n") or not win else None
            starts = [0] + [e + 1 for e in ends[:-1]] if ends else []
            heads = [s for s in starts if win[s:s + 1] == b">"]
            partial = win[ends[-1] + 1:] if ends else win
            carry = win if not heads else partial if partial.startswith(b">") else win[heads[-1]:]
        else:
            done = ends[len(ends) // 4 * 4 - 1] + 1 if len(ends) >= 4 else 0
            carry = win[done:]
            if last:
                return None if carry else carries
        if W is not None and len(carry) > W:
            return None
        carries.append(len(carry))
    return carries


# ---- streams -----------------------------------------------------------------------------------------------------------------
def _one(data, kind):
    if not data:
        return EOF_MEMBER
    if kind == "stored":
        return stored_member(data)
    return member(data, 1 if kind == "level1" else 6)


def stream_of(text, sizes, kinds="level1", eof=True):
    """`text` as members of `sizes` bytes in turn (0: an EOF member where it stands); sum(sizes) == len(text).  `kinds`: one of
    KINDS for all, or one per member.  A stored member holds at most 65 505 bytes: a larger one is made at level 1."""
    assert sum(sizes) == len(text), (sum(sizes), len(text))
    out, at = [], 0
    for k, n in enumerate(sizes):
        kind = kinds if isinstance(kinds, str) else kinds[k]
        if kind == "stored" and n > 65505:
            kind = "level1"
        out.append(_one(text[at:at + n], kind))
        at += n
    return b"".join(out) + (EOF_MEMBER if eof else b"")


def drawn_sizes(rng, total, choices=ISIZES, p_random=0.4):
    """member sizes that sum to `total`: drawn from `choices` and, with p_random, from 1 .. 65 536"""
    sizes, left = [], total
    while left:
        n = rng.randint(1, 65536) if rng.random() < p_random else rng.choice(choices)
        n = min(n, left)
        sizes.append(n)
        left -= n
    return sizes


def drawn_stream(text, seed):
    """-> (blob, sizes): `text` in members of drawn sizes and kinds, EOF members among them, the EOF member last"""
    rng = random.Random(seed)
    sizes = drawn_sizes(rng, len(text))
    kinds = [rng.choice(KINDS) for _ in sizes]
    return stream_of(text, sizes, kinds), sizes


def seeded_member_sets(n_sets=40, seed=20261020):
    """[(isizes, frame sizes)]: member tables alone, for the cut rule — frames from 28 bytes (an EOF member) to 65 536"""
    rng = random.Random(seed)
    out = []
    for _ in range(n_sets):
        M = rng.choice([1, 2, 3, 17, 200, 1500])
        isz, frm = [], []
        for _ in range(M):
            n = rng.choice(ISIZES) if rng.random() < 0.5 else rng.randint(0, 65536)
            ratio = rng.choice([0.0, 0.05, 0.3, 1.0])  # (1.0: stored)
            f = 28 if n == 0 else min(65536, 26 + max(2, int(n * ratio) + (5 if ratio == 1.0 else 0)))
            isz.append(n), frm.append(f)
        out.append((isz, frm))
    return out


def synthetic_stream(isizes, frame_sizes):
    """a stream the walk takes with exactly these ISIZEs and frame sizes (frames >= 26; the payloads are zero bytes: for
    the cut rule, which never decodes)"""
    out = []
    for n, f in zip(isizes, frame_sizes):
        assert 26 <= f <= 65536
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00BC\x02\x00" + struct.pack("<H", f - 1) + b"\0" * (f - 26) + struct.pack("<II", 0, n))
    return b"".join(out)


def borders_of(cuts):
    """the text borders of the windows, for window_carries_at"""
    return [c[5] for c in cuts]
