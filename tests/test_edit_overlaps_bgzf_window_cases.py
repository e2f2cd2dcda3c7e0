"""The overlap editor's windows over a BGZF text (csrc/gpu_edit.hip: bgzf_windows_loop) without a GPU: the
restatement of edit_overlaps_bgzf_window_cases on hand-made streams, the builders of
tests/test_gpu_edit_overlaps_bgzf_windows.py against csrc/bgzf_windows.h (host.bgzf_window_cuts), the restatement of
filter / extract and the host loop, the route's inputs, and — for every seed the GPU file generates a text from — that the
restatement takes every line, so that the GPU test skips nothing."""
import edit_overlaps_bgzf_window_cases as bc
from edit_bgzf_window_cases import cuts_of, stream_of
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, TILE, host_loop, restate
from yacrd_amd import host

W = bc.W_TEST
NEVER = 2 ** 64 - 1
GENERATED = [(20250803 + i, m4, stream) for i, (m4, stream) in enumerate((m4, s) for m4 in (False, True) for s in ("own", "drawn"))]  # the GPU file's
OFFSETS = (0, 1, 63, 64, 65, 127, 128, 129, 32767)


def generated_case(seed, m4, stream, windows=24):
    """-> (text, names, types, blob): the GPU file's generated texts"""
    text, names, types = bc.generated(seed, m4, W, windows=windows)
    blob = bc.own_stream(text, ("stored", "level1", "level6")[seed % 3]) if stream == "own" else bc.drawn(text, seed)
    return text, names, types, blob


def test_the_restatement_on_hand_made_streams():
    #                      window 0 (8 bytes)       window 1 (3)    window 2 (9)
    text = b"abc\ndefg" b"hi\n" b"jklmn\nop\n"
    wins = [(0, 8, 3), (8, 11, 8), (11, 20, 0)]
    assert bc.window_reaches(text, wins) == [3, 0, 0] and bc.refused(text, wins) == []
    assert bc.window_reaches(b"abc\ndefg" b"hij" b"\njklmnop\n", wins) == [4, 0, 0]  # (one byte beyond the three that window 0 sees)
    assert bc.refused(b"abc\ndefg" b"hij" b"\njklmnop\n", wins) == [0]
    assert bc.window_reaches(b"abc\ndefg" b"hij" b"klmnopqrs", wins) == [12, 0, 0]  # (no final newline: the real bytes count)
    assert bc.window_reaches(b"abcdefg\n" b"\n\n\n" b"a\n", [(0, 8, 3), (8, 11, 2), (11, 13, 0)]) == [0, 0, 0]  # (empty lines begin where they lie)
    # the windows are the cuts that hold text; ahead is the next window's bytes, at most C
    cuts = [(0, 1, 0, 10, 0, 60000), (1, 2, 10, 20, 60000, 60000), (2, 3, 20, 30, 60000, 70000), (3, 4, 30, 40, 70000, 135536), (4, 5, 40, 50, 135536, 135536)]
    assert bc.windows_of(cuts, W) == [(0, 60000, 10000), (60000, 70000, 65536), (70000, 135536, 0)]
    assert bc.windows_of(cuts, 2 * W)[0] == (0, 60000, 10000) and bc.windows_of([], W) == []
    assert bc.bgzf_window(1) == W and bc.bgzf_window(W) == W and bc.bgzf_window(W + 1) == W + TILE and bc.bgzf_window(3 * TILE) == 3 * TILE


def test_the_builders_against_the_cut_rule_and_the_host_loop(tmp_path):
    assert "yacrd_bgzf_window_cuts" in host.EXPORTED_SYMBOLS
    for m4 in (False, True):
        text = bc.fill(m4, 60000 + 10000 + 60000, bc.good)
        for eof, empties in ((True, ()), (False, ()), (True, (1,)), (True, (0, 2))):
            blob = bc.with_windows(text, [60000, 10000, 60000], eof=eof, empties=empties)
            cuts = cuts_of(blob, W)
            assert [tuple(c) for c in host.bgzf_window_cuts(blob, W)] == cuts
            assert [(w[1] - w[0], w[2]) for w in bc.windows_of(cuts, W)] == [(60000, 10000), (10000, 60000), (60000, 0)]
        # stored members of 65 505 bytes: a frame of 65 536 fills the window's stream cap, the EOF member is a cut of its own
        blob = bc.with_windows(bc.fill(m4, 2 * 65505, bc.bad), [65505, 65505])
        cuts = cuts_of(blob, W)
        assert cuts[-1][5] == cuts[-1][4] and cuts[-1][1] - cuts[-1][0] == 1 and len(bc.windows_of(cuts, W)) == 2
        for off in OFFSETS:
            for op, want_kept in ((OP_FILTER, True), (OP_EXTRACT, False)):
                cases = bc.border_sweep(m4, off, want_kept, op)
                assert [c for c, _, _ in cases] == list(range(101))
                for cut, text, T in cases[::50]:
                    assert T % TILE == off and len(text) == T + bc.SWEEP_NEXT
                    blob = bc.with_windows(text, [T, bc.SWEEP_NEXT])
                    wins = bc.windows_of(cuts_of(blob, W), W)
                    assert wins == [(0, T, bc.SWEEP_NEXT), (T, len(text), 0)] and bc.window_reaches(text, wins)[0] == (101 - cut if cut else 0)
                    kept, n_lines, n_kept = restate(text, op, bc.TABLE, m4)
                    target = text[T - cut:T - cut + 101]
                    assert target.count(b"\n") == 1 and target.endswith(b"\n") and text[T - cut - 1:T - cut] == b"\n"
                    assert (target in kept) == want_kept and 0 < n_kept < n_lines
                    assert kept == host_loop(str(tmp_path), op, text, bc.NAMES, bc.TYPES, ".m4" if m4 else ".paf")
        # the look-ahead's edge: ahead == C behind a full window, and a short next window
        for lens, T, ahead in (([W, W, 1000], W, W), ([60000, 10000, 60000], 60000, 10000)):
            for reach, take in ((ahead - 1, True), (ahead, True), (ahead + 1, False)):
                text = bc.reaching(m4, T, reach, behind=sum(lens) - T - reach)
                assert len(text) == sum(lens)
                blob = bc.with_windows(text, lens)
                wins = bc.windows_of(cuts_of(blob, W), W)
                assert wins[0][2] == ahead and bc.window_reaches(text, wins)[0] == reach and bc.windows_take(text, blob, W) is take


def test_every_line_of_the_generated_texts_is_taken(tmp_path):
    """zero refusals for the GPU file's seeds, at its windows"""
    for seed, m4, stream in GENERATED:
        text, names, types, blob = generated_case(seed, m4, stream)
        assert host.bgzf_decode_host(blob) == text
        for w in (W, W + TILE, 2 * W):
            cuts = cuts_of(blob, w)
            assert [tuple(c) for c in host.bgzf_window_cuts(blob, w)] == cuts
            wins = bc.windows_of(cuts, w)
            assert bc.refused(text, wins) == [] and len(wins) >= 10, (seed, w)
        assert 20 <= len(bc.windows_of(cuts_of(blob, W), W)) <= 40
        kept = restate(text, OP_FILTER, dict(zip(names, types)), m4)
        assert 0 < kept[2] < kept[1]
        if stream == "own":
            assert kept[0] == host_loop(str(tmp_path), OP_FILTER, text, names, types, ".m4" if m4 else ".paf")


def test_the_route_inputs():
    """edit_route.h decides over the same four inputs; a BGZF run hands it a switch of at least 64 KiB"""
    seg = 128 << 20
    assert host.edit_window_route(40 * seg, 0, False, True)[0] == host.EDIT_WINDOWS  # (no room whole: windows, not the host loop)
    assert host.edit_window_route(40 * seg, 0, True, True)[0] == host.EDIT_WHOLE  # (the BGZF when-fits constant is false)
    assert host.edit_window_route(40 * seg, NEVER, False, True)[0] == host.EDIT_FALLBACK
    # a switch of one tile is raised to 64 KiB for a BGZF text: a text of 50 000 bytes is one window and runs whole
    assert bc.bgzf_window(TILE) == W and host.edit_window_route(50000, bc.bgzf_window(TILE), True, True)[0] == host.EDIT_WHOLE
    assert host.edit_window_route(W + 1, bc.bgzf_window(TILE), True, True) == (host.EDIT_WINDOWS, W, W)
