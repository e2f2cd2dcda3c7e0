"""The overlap editor's windows (csrc/gpu_edit.hip: windows_loop) without a GPU: the windows' rule restated in
edit_overlaps_window_cases on hand-made texts, the generators of tests/test_gpu_edit_overlaps_windows.py against the
restatement of filter / extract and the host loop, and the route — whole text, windows of W, or fall back — that
csrc/edit_route.h decides and yacrd_amd/host.py binds, over its four inputs."""
import itertools

import edit_overlaps_window_cases as wc
from edit_overlaps_cases import CHUNK, OP_EXTRACT, OP_FILTER, TILE, host_loop, restate
from yacrd_amd import host

W = wc.W_TEST
NEVER = 2 ** 64 - 1


def test_the_rule_on_hand_made_texts():
    assert wc.chunk_of(TILE) == TILE and wc.chunk_of(3 * TILE) == 3 * TILE and wc.chunk_of(CHUNK + TILE) == CHUNK
    assert wc.window_reaches(b"", 8) == [] and wc.windows_take(b"", 8) is True
    #                         window 0  | window 1 | window 2
    assert wc.window_reaches(b"abc\ndefg" b"hi\njklmn" b"\n", 8) == [3, 1, 0]
    assert wc.window_reaches(b"abc\ndef\n" b"hi\njklm\n", 8) == [0, 0]  # (lines end on the borders: nothing reaches)
    assert wc.window_reaches(b"abc\ndefg" b"hijklmno" b"pq", 8) == [10, 0, 0]  # (no final newline: the real bytes count)
    assert wc.window_reaches(b"abcdefg\n" b"\n\n", 8) == [0, 0]  # (empty lines begin where they lie)
    # C = W for a window of at most 4 MiB: a line may fill the next window to its last byte, not one byte more
    for reach, take in ((W - 1, True), (W, True), (W + 1, False)):
        for newline in (True, False):
            text = wc.reaching(False, W, reach, newline=newline, behind=False)
            assert wc.windows_take(text, W) is take, (reach, newline)
    assert wc.windows_take(b'a\t"b"\n', W) is None and wc.windows_take(b"a\r\n", W) is None
    # a line of at most C + 1 bytes is taken wherever it lies
    line = wc.good(True, W) + b"\n"
    for lead in (0, 1, W - 1, W, 2 * W - 1):
        assert wc.windows_take(wc.fill(True, lead, wc.bad) + line if lead >= 60 else b"\n" * lead + line, W)


def test_the_generators_hold_what_they_say(tmp_path):
    names = wc.NAMES
    for m4 in (False, True):
        ext = ".m4" if m4 else ".paf"
        for maker, kept_by in ((wc.good, OP_FILTER), (wc.bad, OP_EXTRACT)):
            l = maker(m4) + b"\n"
            for op in (OP_FILTER, OP_EXTRACT):
                assert restate(l, op, wc.TABLE, m4)[0] == (l if op == kept_by else b"")
            assert len(wc.fill(m4, 12345, maker)) == 12345 and wc.fill(m4, 0) == b""
        text, known, types = wc.generated(7, m4, W, windows=3)
        assert len(text) == 3 * W - 777 and wc.windows_take(text, W) and wc.n_windows(text, W) == 3
        assert restate(text, OP_FILTER, dict(zip(known, types)), m4)[0] == host_loop(str(tmp_path), OP_FILTER, text, known, types, ext)
        for op, want_kept in itertools.product((OP_FILTER, OP_EXTRACT), (True, False)):
            cases = wc.border_sweep(m4, W, want_kept, op)
            assert [c for c, _ in cases] == list(range(101))
            for cut, text in cases[::20] + cases[-1:]:
                kept, n_lines, n_kept = restate(text, op, wc.TABLE, m4)
                target = text[W - cut:W - cut + 101]
                assert target.endswith(b"\n") and target.count(b"\n") == 1 and text[W - cut - 1:W - cut] == b"\n"
                assert (target in kept) == want_kept and 0 < n_kept < n_lines
                assert wc.n_windows(text, W) == 2 and wc.windows_take(text, W)
                assert kept == host_loop(str(tmp_path), op, text, names, wc.TYPES, ext)
        for target in (wc.good, wc.bad):
            text = wc.no_start_window(m4, W, target)
            reaches = wc.window_reaches(text, W)  # (window 0's: a short line across the first border)
            assert reaches[1:] == [W, 0, 0] and reaches[0] < 200 and wc.windows_take(text, W)
            for op in (OP_FILTER, OP_EXTRACT):
                kept = restate(text, op, wc.TABLE, m4)[0]
                assert kept == host_loop(str(tmp_path), op, text, names, wc.TYPES, ext)
                assert (len(kept) == W + 1) == ((target is wc.good) == (op == OP_FILTER))  # (the long line alone, or all the others)


def test_the_route_over_its_four_inputs():
    assert "yacrd_edit_window_route" in host.EXPORTED_SYMBOLS
    seg = 128 << 20
    for sw, want_w in ((0, seg), (NEVER, seg), (1, TILE), (TILE, TILE), (TILE + 1, 2 * TILE), (CHUNK + 5, CHUNK + TILE), (3 * seg, 3 * seg)):
        _, w, c = host.edit_window_route(0, sw, True, True)
        assert (w, c) == (want_w, min(CHUNK, want_w)), sw
    for sw, whole, ring in itertools.product((0, NEVER, TILE, 5 * TILE, seg, 2 * seg), (True, False), (True, False)):
        w = host.edit_window_route(0, sw, whole, ring)[1]
        for n in (0, 1, w - 1, w, w + 1, 2 * w, 40 * w + 3):
            got = host.edit_window_route(n, sw, whole, ring)[0]
            if n <= w or sw == NEVER:  # at most one window, or never windows: as before the windows
                want = host.EDIT_WHOLE if whole else host.EDIT_FALLBACK
            elif sw != 0 or not whole:  # the switch names a window, or the whole text finds no room: windows, if the ring fits
                want = host.EDIT_WINDOWS if ring else host.EDIT_FALLBACK
            else:  # the policy and room for the whole text (kEdWindowsWhenFits is false: DESIGN 7n)
                want = host.EDIT_WHOLE
            assert got == want, (n, sw, whole, ring)
    # the case the windows are for: no room whole, the policy -> windows instead of the host loop
    assert host.edit_window_route(40 * seg, 0, False, True)[0] == host.EDIT_WINDOWS
    assert host.edit_window_route(40 * seg, NEVER, False, True)[0] == host.EDIT_FALLBACK
