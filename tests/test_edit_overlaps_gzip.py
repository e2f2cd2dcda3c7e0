"""CPU half of filter / extract with gzip out on the device (tests/test_gpu_edit_overlaps_gzip.py is the GPU half): the library
exports the two entry points, the binding is there, and the yardstick the GPU tests compare members with — the host build
of the encoder over the host loop's kept bytes — is a well-formed BGZF stream of those bytes on the seam sizes."""
import ctypes
import gzip
import random

import yacrd_amd
from deflate_cases import BLOCK, EOF_MEMBER, walk_bgzf
from edit_overlaps_cases import OP_EXTRACT, OP_FILTER, restate
from edit_overlaps_gzip_cases import seam_text
from yacrd_amd import host

NEW_SYMBOLS = ["yacrd_engine_edit_overlaps_gzip_mem", "yacrd_engine_edit_overlaps_gzip_file"]


def test_the_library_exports_the_gzip_editor():
    lib = ctypes.CDLL(yacrd_amd.lib_path())
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in yacrd_amd.EXPORTED_SYMBOLS, n
    assert callable(getattr(yacrd_amd.Engine, "edit_overlaps_gzip", None))
    assert yacrd_amd.load_library().yacrd_abi_version() == 7


def test_seam_texts_keep_what_they_say():
    """the seam generator: the kept bytes of the text are exactly the size asked for, for both ops and both formats"""
    rng = random.Random(7)
    for m4 in (False, True):
        for op in (OP_FILTER, OP_EXTRACT):
            for size in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK):
                text, names, types = seam_text(rng, op, m4, size)
                kept, n_lines, n_kept = restate(text, op, dict(zip(names, types)), m4)
                assert len(kept) == size and 0 < n_kept < n_lines
                blob = host.bgzf_encode_host(kept)
                members = walk_bgzf(blob)
                assert [len(d) for _, d in members] == [BLOCK] * (size // BLOCK) + ([size % BLOCK] if size % BLOCK else []) + [0]
                assert members[-1][0] == EOF_MEMBER and gzip.decompress(blob) == kept
