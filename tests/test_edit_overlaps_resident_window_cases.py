"""The overlap editor's windows over a resident text (csrc/gpu_edit.hip: windows_loop from the mirror) without a
GPU: the generators of tests/test_gpu_edit_overlaps_resident_windows.py hold what they say — every text is a text the host
parser takes record by record (an ingest comes first), the restatement and the host loop agree on it, and the windows' rule
(edit_overlaps_window_cases) takes every line of every text the GPU file expects to be taken and refuses the ones it expects
to be refused — and the route (csrc/edit_route.h) over the inputs the resident forms give it."""
import itertools

import edit_overlaps_resident_window_cases as rc
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, TILE, host_loop, restate
from yacrd_amd import host

W = rc.W_TEST
C = rc.chunk_of(W)
NEVER = 2 ** 64 - 1
GENERATED_SEEDS = (20250710, 20250711)  # the GPU file's: seed + m4


def _records(text, m4):
    """overlaps the host parser makes of `text` (every record counts twice: once for each read)"""
    csr = host.csr_from_memory(text, 2 if m4 else 1)
    try:
        return int(csr.offsets[-1]) // 2
    finally:
        csr.close()


def _lines(text):
    return sum(1 for l in text.split(b"\n") if l)


def test_lines_are_records_and_verdicts_are_what_the_makers_say(tmp_path):
    for m4 in (False, True):
        ext = ".m4" if m4 else ".paf"
        for maker, kept_by in ((rc.good, OP_FILTER), (rc.bad, OP_EXTRACT)):
            for size in (None, 100, 3 * W):  # (stretched by leading zeros: still one record)
                l = maker(m4, size) + b"\n"
                assert size is None or len(l) == size + 1
                assert _records(l, m4) == 1
                for op in (OP_FILTER, OP_EXTRACT):
                    assert restate(l, op, rc.TABLE, m4)[0] == (l if op == kept_by else b"")
            assert len(rc.fill(m4, 12345, maker)) == 12345 and rc.fill(m4, 0) == b""
        text = rc.generated(7, m4, W, windows=3)
        assert len(text) == 3 * W - 777 and rc.n_windows(text, W) == 3 and _records(text, m4) == _lines(text)
        for op in (OP_FILTER, OP_EXTRACT):
            kept, n_lines, n_kept = restate(text, op, rc.TABLE, m4)
            assert 0 < n_kept < n_lines and kept == host_loop(str(tmp_path), op, text, rc.NAMES, rc.TYPES, ext)


def test_every_line_of_the_generated_texts_is_taken():
    """the seeds of the GPU file's generated test: zero refusals, so that test may skip nothing"""
    for m4 in (False, True):
        text = rc.generated(GENERATED_SEEDS[m4], m4, W)
        reaches = rc.window_reaches(text, W)
        assert len(reaches) == 40 and rc.windows_take(text, W) is True and 0 < max(reaches) <= C
        assert _records(text, m4) == _lines(text) and b"\n\n" in text  # (every non-empty line a record; empty lines among them)
        kept = restate(text, OP_FILTER, rc.TABLE, m4)
        assert 0 < kept[2] < kept[1]


def test_the_shaped_texts(tmp_path):
    for m4 in (False, True):
        ext = ".m4" if m4 else ".paf"
        for op, want_kept in itertools.product((OP_FILTER, OP_EXTRACT), (True, False)):
            cases = rc.border_sweep(m4, W, want_kept, op)
            assert [c for c, _ in cases] == list(range(101))
            for cut, text in cases[::25] + cases[-1:]:
                kept, n_lines, n_kept = restate(text, op, rc.TABLE, m4)
                target = text[W - cut:W - cut + 101]
                assert target.endswith(b"\n") and target.count(b"\n") == 1 and text[W - cut - 1:W - cut] == b"\n"
                assert (target in kept) == want_kept and 0 < n_kept < n_lines
                assert rc.n_windows(text, W) == 2 and rc.windows_take(text, W) and _records(text, m4) == n_lines
                assert rc.window_reaches(text, W)[0] == (101 - cut if cut else 0)
                assert kept == host_loop(str(tmp_path), op, text, rc.NAMES, rc.TYPES, ext)
        for target in (rc.good, rc.bad):
            text = rc.no_start_window(m4, W, target)
            assert rc.window_reaches(text, W)[1:] == [W, 0, 0] and rc.windows_take(text, W) and _records(text, m4) == _lines(text)
        # the look-ahead's edge, behind window 0 and behind window 8: C - 1 and C are taken, C + 1 is not
        for lead, (reach, take), newline in itertools.product((1, 9), ((C - 1, True), (C, True), (C + 1, False)), (True, False)):
            text = rc.reaching(m4, W, reach, newline=newline, behind=False, lead_windows=lead)
            assert rc.windows_take(text, W) is take and _records(text, m4) == _lines(text), (lead, reach, newline)
            assert rc.window_reaches(text, W)[lead - 1] == reach and max(rc.window_reaches(text, W)) == reach


def test_the_route_with_the_text_left_out():
    """The resident forms and the edit from the mirror hand edit_route.h the same four inputs as a plain text does; what
    differs is what the two `fits` count (the text is in neither need) — the decision over them is the one function."""
    seg = 128 << 20
    # a resident text of 40 segments that finds no room for 1.125 n of output beside the detection's buffers: windows
    assert host.edit_window_route(40 * seg, 0, False, True) == (host.EDIT_WINDOWS, seg, 4 << 20)
    assert host.edit_window_route(40 * seg, 0, True, True)[0] == host.EDIT_WHOLE  # (room: as before)
    assert host.edit_window_route(40 * seg, NEVER, False, True)[0] == host.EDIT_FALLBACK
    assert host.edit_window_route(40 * seg, 0, False, False)[0] == host.EDIT_FALLBACK
    # the tests' switch: 32 768 names a window of one tile with a look-ahead of one tile; a text of one window runs whole
    assert host.edit_window_route(40 * TILE - 777, TILE, True, True) == (host.EDIT_WINDOWS, TILE, TILE)
    assert host.edit_window_route(TILE, TILE, True, True)[0] == host.EDIT_WHOLE
    assert host.edit_window_route(TILE + 1, TILE, True, True)[0] == host.EDIT_WINDOWS
