"""filter / extract on overlap files, the part that needs no GPU: the new entry points are exported, and the ten-line
restatement of the rule that the GPU tests count with equals the host loop on the whole fuzz set."""
import ctypes

import numpy as np

import yacrd_amd
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, fuzz_cases, host_loop, restate

NEW_SYMBOLS = ["yacrd_engine_edit_overlaps", "yacrd_engine_edit_overlaps_mem", "yacrd_edit_text_free"]


def test_the_library_exports_the_overlap_editor():
    lib = ctypes.CDLL(yacrd_amd.lib_path())
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in yacrd_amd.EXPORTED_SYMBOLS, n
    assert callable(getattr(yacrd_amd.Engine, "edit_overlaps", None))
    assert callable(getattr(yacrd_amd.Engine, "edit_overlaps_text", None))


def test_the_restatement_is_the_host_loop(tmp_path):
    n = 0
    for tag, text, m4, names, types in fuzz_cases():
        table = dict(zip(names, types))
        for op in (OP_FILTER, OP_EXTRACT):
            want = host_loop(str(tmp_path), op, text, names, types, ".m4" if m4 else ".paf")
            got, n_lines, n_kept = restate(text, op, table, m4)
            assert got == want, (tag, m4, op)
            assert n_kept == got.count(b"\n") and n_kept <= n_lines
        n += 1
    assert n >= 1000


def test_the_fuzz_set_has_what_it_says():
    tags = {}
    some_kept = some_dropped = absent = 0
    for tag, text, m4, names, types in fuzz_cases():
        tags.setdefault(tag.rstrip("0123456789"), 0)
        got, n_lines, n_kept = restate(text, OP_FILTER, dict(zip(names, types)), m4)
        some_kept += 0 < n_kept
        some_dropped += n_kept < n_lines
        ids = {l.split(b" " if m4 else b"\t")[0] for l in text.split(b"\n") if l}
        absent += bool(ids - set(names))
        assert all(1 <= len(x) <= 300 for x in names)
    assert some_kept > 300 and some_dropped > 300 and absent > 300
    assert {"small", "empty", "one", "one_open"} <= set(tags)
    assert any(len(t) > 4 << 20 for _, t, _, _, _ in fuzz_cases(n_small=0))
    assert np.unique([len(t) for _, t, _, _, _ in fuzz_cases(n_small=0)]).size > 30
