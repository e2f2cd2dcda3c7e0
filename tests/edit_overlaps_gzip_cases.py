"""What tests/test_edit_overlaps_gzip.py (CPU) and tests/test_gpu_edit_overlaps_gzip.py (GPU) share: texts whose KEPT size is
known in advance, for the seams of the 65 280-byte blocks the kept stream is deflated in."""
from edit_overlaps_cases import OP_FILTER, _line, _sized, _token


def seam_text(rng, op, m4, kept_size):
    """-> (text, names, types): a text of which `op` keeps exactly `kept_size` bytes.  The lines to keep come from _sized
    (its empty lines taken out, the last line stretched by what they took), lines to drop lie between them."""
    good = sorted({_token(rng, rng.choice([1, 3, 8, 21, 40])) for _ in range(6)})
    bad = sorted({b"!" + _token(rng, rng.choice([1, 5, 13, 80])) for _ in range(4)})  # ('!' is not in the alphabet: no id is both)
    keep_ids, drop_ids = (good, bad) if op == OP_FILTER else (bad, good)
    cols = rng.randint(9, 17)
    lines = [l for l in _sized(rng, keep_ids, cols, m4, kept_size).split(b"\n") if l]
    lines[-1] += b"x" * (kept_size - sum(len(l) + 1 for l in lines))
    assert sum(len(l) + 1 for l in lines) == kept_size
    parts = []
    for l in lines:
        while rng.random() < 0.3:
            parts.append(_line(rng, drop_ids, cols, m4))
        if rng.random() < 0.05:
            parts.append(b"")
        parts.append(l)
    parts.append(_line(rng, drop_ids, cols, m4))
    names = good[:3] + bad  # (some good ids are absent from the table: absent is NotBad)
    types = [0] * 3 + [1 + i % 2 for i in range(len(bad))]
    return b"\n".join(parts) + b"\n", names, types
