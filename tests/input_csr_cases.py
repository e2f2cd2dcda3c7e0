"""What tests/test_input_csr_cases.py (CPU) and tests/test_gpu_input_csr.py (GPU) share: the comparison of an input CSR — the
offsets / intervals / lengths the sweeps consume — with a reference, interval by interval, the reference CSR of raw overlap
records, and seeded record generators on the edges of the build on the GPU (csrc/csr_build.h: wavefronts of 64 records,
workgroups of 256, runs of equal ids, scan tiles of 4096 reads).  numpy only: nothing here runs the oracle or the engine."""
import functools

import numpy as np

REC_DTYPE = np.dtype([(n, np.uint32) for n in ("a", "b", "sa", "ea", "sb", "eb")])  # == yacrd_amd.OVL_REC_DTYPE (yacrd_ovl_rec)
READ_LENGTH = 100000  # every generated read's length; coordinates lie inside it


# ---- the comparison -------------------------------------------------------------------------------------------------------
def assert_same_csr(got, want, ctx="", exact=False):
    """got: Engine.debug_input_csr()'s (offsets, intervals, lengths), or None; want: the reference's.  Offsets and lengths
    must be equal, and every read must hold the same multiset of (start, end) rows — in the same order too when `exact`."""
    assert got is not None, "%s: the engine has no input CSR to show" % ctx
    g_off, g_iv, g_len = (np.asarray(x) for x in got)
    w_off, w_iv, w_len = (np.asarray(x) for x in want)
    g_iv, w_iv = g_iv.reshape(-1, 2), w_iv.reshape(-1, 2)
    if g_off.shape != w_off.shape:
        raise AssertionError("%s: %d reads, want %d" % (ctx, len(g_off) - 1, len(w_off) - 1))
    if not np.array_equal(g_off.astype(np.uint64), w_off.astype(np.uint64)):
        g_n, w_n = np.diff(g_off.astype(np.int64)), np.diff(w_off.astype(np.int64))
        differ = np.nonzero(g_n != w_n)[0]
        if len(differ) == 0:  # (the counts agree: offsets[0] is not 0)
            raise AssertionError("%s: offsets start at %d, want %d" % (ctx, int(g_off[0]), int(w_off[0])))
        r = int(differ[0])
        raise AssertionError("%s: interval count differs first at read %d: got %d want %d (%d reads differ)" % (
            ctx, r, int(g_n[r]), int(w_n[r]), len(differ)))
    total = int(w_off[-1]) if len(w_off) else 0
    if len(g_iv) != total or len(w_iv) != total:
        raise AssertionError("%s: %d interval rows (the reference: %d) under offsets that end at %d" % (ctx, len(g_iv), len(w_iv), total))
    if not np.array_equal(g_len.astype(np.uint64), w_len.astype(np.uint64)):
        r = int(np.nonzero(g_len.astype(np.uint64) != w_len.astype(np.uint64))[0][0])
        raise AssertionError("%s: length differs first at read %d: got %d want %d" % (ctx, r, int(g_len[r]), int(w_len[r])))
    differ = (g_iv != w_iv).any(axis=1)
    if not differ.any():
        return
    n = np.diff(w_off.astype(np.int64))
    read_id = np.repeat(np.arange(len(n), dtype=np.int64), n)
    if not exact:
        # a read whose rows are equal one by one holds the same multiset: sort (read, start, end) only the rows of the others
        touched = np.zeros(len(n), dtype=bool)
        touched[read_id[differ]] = True
        rows = touched[read_id]
        read_id, g_iv, w_iv = read_id[rows], g_iv[rows], w_iv[rows]
        g_iv = g_iv[np.lexsort((g_iv[:, 1], g_iv[:, 0], read_id))]
        w_iv = w_iv[np.lexsort((w_iv[:, 1], w_iv[:, 0], read_id))]
        differ = (g_iv != w_iv).any(axis=1)
        if not differ.any():
            return
    r = int(read_id[np.argmax(differ)])
    raise AssertionError("%s: the intervals of read %d differ%s (%d of its %d rows):\n  got  %s\n  want %s" % (
        ctx, r, " in value or order" if exact else "", int(differ[read_id == r].sum()), int(n[r]),
        g_iv[read_id == r].tolist(), w_iv[read_id == r].tolist()))


def assert_same_csr_in_ranges(parts, want, ctx=""):
    """parts: the input CSRs of the engines of a group that holds the reads in ranges (the N-engine device parser), in engine
    order; want: the whole reference CSR.  End to end they are `want`, and every engine holds as many intervals as its reads
    count."""
    for k, part in enumerate(parts):
        assert part is not None, "%s: engine %d has no input CSR to show" % (ctx, k)
    w_off = np.asarray(want[0]).astype(np.uint64)
    lo = 0
    for k, (off, iv, ln) in enumerate(parts):
        hi = lo + len(ln)
        assert hi < len(w_off), "%s: engines 0..%d hold %d reads of %d" % (ctx, k, hi, len(w_off) - 1)
        share = int(w_off[hi] - w_off[lo])
        assert len(iv) == int(off[-1]) == share, "%s: engine %d (reads %d..%d) holds %d intervals, offsets end at %d, its share is %d" % (
            ctx, k, lo, hi, len(iv), int(off[-1]), share)
        lo = hi
    ends = np.cumsum([0] + [int(off[-1]) for off, _, _ in parts]).astype(np.uint64)
    offsets = np.concatenate([np.zeros(1, np.uint64)] + [off[1:].astype(np.uint64) + ends[k] for k, (off, _, _) in enumerate(parts)])
    assert_same_csr((offsets, np.concatenate([iv for _, iv, _ in parts]), np.concatenate([ln for _, _, ln in parts])), want, ctx)


# ---- the reference for raw records ----------------------------------------------------------------------------------------
def csr_of_records(recs, n_reads, handle_map=None, keep=None):
    """Overlap records -> (offsets u64[R + 1], intervals u32[I, 2]): both halves of every record go to the read its handle
    maps to (the identity without a map), a read's intervals in record order.  `keep` (bool per read): one engine's share of a
    group — only those reads, numbered in order, and only the halves that name them."""
    a, b = recs["a"].astype(np.int64), recs["b"].astype(np.int64)
    if handle_map is not None:
        handle_map = np.asarray(handle_map, dtype=np.int64)
        a, b = handle_map[a], handle_map[b]
    read_id = np.stack([a, b], axis=1).reshape(-1)
    rows = np.stack([recs["sa"], recs["ea"], recs["sb"], recs["eb"]], axis=1).reshape(-1, 2).astype(np.uint32)
    assert read_id.size == 0 or (0 <= read_id.min() and read_id.max() < n_reads)
    if keep is not None:
        keep = np.asarray(keep, dtype=bool)
        local = np.cumsum(keep) - 1  # read -> its number among the kept
        mine = keep[read_id]
        read_id, rows, n_reads = local[read_id[mine]], rows[mine], int(keep.sum())
    offsets = np.zeros(n_reads + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(read_id, minlength=n_reads))
    return offsets, rows[np.argsort(read_id, kind="stable")]


def handle_of_read(handle_map, n_reads):
    """read -> the handle that maps to it, for a map that is one-to-one onto the reads (0xFFFFFFFF: a handle no record uses)"""
    handle_map = np.asarray(handle_map, dtype=np.int64)
    used = np.nonzero(handle_map != 0xFFFFFFFF)[0]
    inv = np.full(n_reads, -1, np.int64)
    inv[handle_map[used]] = used
    assert len(used) == n_reads and (inv >= 0).all()
    return inv


def kept_reads(csr, keep):
    """the reads of `csr` where `keep` (bool per read) holds, in order: one engine's share of a group"""
    offsets, intervals, lengths = csr
    n = np.diff(offsets.astype(np.int64))
    out = np.zeros(int(keep.sum()) + 1, np.uint64)
    out[1:] = np.cumsum(n[keep])
    return out, intervals[np.repeat(keep, n)], lengths[keep]


# ---- the five ways one interval goes wrong (the CPU test shows the comparison reports every one) ----------------------------
MUTATIONS = ("end_plus_1", "start_plus_7", "dropped", "duplicated", "another_reads")


def mutate(csr, kind, k, rng):
    """`csr` with its interval k damaged: a copy; lengths untouched"""
    offsets, intervals, lengths = csr
    offsets, intervals = offsets.copy(), intervals.copy()
    r = int(np.searchsorted(offsets, np.uint64(k), side="right") - 1)
    if kind == "end_plus_1":
        intervals[k, 1] += 1
    elif kind == "start_plus_7":
        intervals[k, 0] += 7
    elif kind == "dropped":
        intervals = np.delete(intervals, k, axis=0)
        offsets[r + 1:] -= np.uint64(1)
    elif kind == "duplicated":
        intervals = np.insert(intervals, k, intervals[k], axis=0)
        offsets[r + 1:] += np.uint64(1)
    elif kind == "another_reads":  # the row of an interval of some other read, which differs from this one
        while True:
            j = int(rng.integers(len(intervals)))
            if not (offsets[r] <= j < offsets[r + 1]) and tuple(intervals[j]) != tuple(intervals[k]):
                break
        intervals[k] = intervals[j]
    else:
        raise ValueError(kind)
    return offsets, intervals, lengths


def shuffled_inside_reads(csr, rng):
    """the same CSR, every read's rows in a random order"""
    offsets, intervals, lengths = csr
    n = np.diff(offsets.astype(np.int64))
    read_id = np.repeat(np.arange(len(n)), n)
    return offsets, intervals[np.lexsort((rng.random(len(intervals)), read_id))], lengths


# ---- record generators ----------------------------------------------------------------------------------------------------
def records(a, b, seed):
    """records between the handles a[i] and b[i]; random coordinates, start < end <= READ_LENGTH"""
    rng = np.random.default_rng(seed)
    recs = np.zeros(len(a), dtype=REC_DTYPE)
    recs["a"], recs["b"] = a, b
    for side in "ab":
        start = rng.integers(0, READ_LENGTH - 1, len(a))
        recs["s" + side] = start
        recs["e" + side] = rng.integers(start + 1, READ_LENGTH + 1)
    return recs


def _runs(*segments):
    """(id, count), ... -> the ids of the `a` column, record by record: lane i of the build's wavefronts holds record i"""
    return np.concatenate([np.full(n, i, dtype=np.int64) for i, n in segments])


COUNT_EDGES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)  # records: wavefronts of 64, workgroups of 256; the last wavefront partly idle
READ_COUNT_EDGES = (1, 4095, 4096, 4097, 8193)         # reads: the scan's tiles hold 4096


@functools.lru_cache(maxsize=None)
def stream_cases():
    """-> {name: (records, n_reads, handle_map or None)}: small batches for the streaming build, count pass included"""
    rng = np.random.default_rng(20260101)
    out = {}
    for n in COUNT_EDGES:  # ids in sorted runs, as in a PAF grouped by query
        out["records_%d" % n] = (records(np.sort(rng.integers(0, 37, n)), rng.integers(0, 37, n), 100 + n), 37, None)

    def with_runs(name, a, n_reads=12, b=None):
        b = rng.integers(0, n_reads, len(a)) if b is None else b
        out[name] = (records(a, b, len(out)), n_reads, None)

    with_runs("runs_of_one", rng.permutation(300), 300)                          # no two neighbours equal
    with_runs("run_of_64_from_lane_0", _runs((5, 64), (6, 64), (7, 10)))
    with_runs("run_of_64_from_lane_1", _runs((1, 1), (5, 64), (2, 70)))
    with_runs("run_head_on_lane_63", _runs((1, 63), (5, 40), (2, 30)))
    with_runs("run_of_one_on_lane_63", _runs((1, 63), (5, 1), (6, 65), (7, 62), (8, 3)))
    with_runs("run_of_200_over_four_wavefronts", _runs((3, 100), (9, 200), (4, 20)))  # records 100 .. 299: past the workgroup edge at 256
    with_runs("all_records_one_read", np.zeros(300, np.int64), 3, np.zeros(300, np.int64))
    with_runs("alternating_ids", np.arange(300) % 2, 2)
    with_runs("self_overlap_alone", np.array([1]), 3, np.array([1]))
    run = _runs((2, 30), (4, 100), (7, 30))
    with_runs("self_overlaps_inside_a_run", run, 12, np.where(np.arange(len(run)) % 3 == 0, run, (run + 5) % 12))
    a, b = np.sort(rng.integers(0, 150, 700)), rng.integers(0, 150, 700)
    out["map_permutes"] = (records(a, b, 7001), 150, rng.permutation(150).astype(np.uint32))
    a, b = np.sort(rng.integers(0, 500, 700)), rng.integers(0, 500, 700)
    out["map_many_handles_to_one_read"] = (records(a, b, 7002), 7, (np.arange(500) % 7).astype(np.uint32))
    for R in READ_COUNT_EDGES:  # most reads empty: zero counts on both sides of a scan tile's edge, the last read not empty
        ids = np.array(sorted({r for r in (0, 1, 4093, 4095, 4096, 4097, 8190, 8191, 8192, R - 1) if r < R}))
        a, b = np.sort(rng.choice(ids, 200)), rng.choice(ids, 200)
        a[-1] = b[0] = R - 1
        out["reads_%d" % R] = (records(a, b, 8000 + R), R, None)
    return out


BIG_READS = 1025 * 4096 + 1  # more than 1024 scan tiles: the carry loop of scan_parts_kernel takes a second trip
BIG_RECORDS = 1_150_000      # more than the 256 * 16 * 256 records one grid of the count / scatter kernels covers at once


def big_stream_case():
    """-> (records, n_reads): `a` in sorted runs of 10 over every tile of the scan, `b` anywhere; the first and the last
    read and both sides of the 1024th tile's edge hold intervals.  Built vectorised; not cached (~30 MB)."""
    rng = np.random.default_rng(4198401)
    heads = np.sort(rng.choice(BIG_READS, BIG_RECORDS // 10, replace=False))
    a = np.repeat(heads, 10)
    b = rng.integers(0, BIG_READS, BIG_RECORDS)
    b[:6] = (0, BIG_READS - 1, 1024 * 4096 - 1, 1024 * 4096, 1025 * 4096 - 1, 1025 * 4096)
    return records(a, b, 4198402), BIG_READS


@functools.lru_cache(maxsize=None)
def group_case():
    """-> (records, n_reads, handle_map): for N engines (a read belongs to engine handle % N): records whose two reads fall on
    one engine and on two for every N in 2, 3, 5, self-overlaps, runs; the map permutes (one-to-one, as a group demands)"""
    rng = np.random.default_rng(606)
    R, n = 211, 3000
    a = np.sort(rng.integers(0, R, n))
    b = rng.integers(0, R, n)
    b[::7] = a[::7]                       # self-overlaps
    b[1::7] = (a[1::7] + 30) % R          # a multiple of 2, 3 and 5 apart: the same engine whatever N
    return records(a, b, 607), R, rng.permutation(R).astype(np.uint32)


UPLOAD_PIECE = 4 << 20  # yke::h2d moves pageable arrays in pieces of 4 MiB through 12 pinned buffers
UPLOAD_BYTES = (UPLOAD_PIECE - 8, UPLOAD_PIECE, UPLOAD_PIECE + 8, 3 * UPLOAD_PIECE + 8, 13 * UPLOAD_PIECE + 8)


def upload_case(n_bytes):
    """-> a CSR whose interval array is n_bytes long: random u32 contents, reads of 100 intervals (the last one the rest)"""
    assert n_bytes % 8 == 0
    n_iv = n_bytes // 8
    rng = np.random.default_rng(n_bytes)
    intervals = rng.integers(0, 2**32, size=(n_iv, 2), dtype=np.uint64).astype(np.uint32)
    offsets = np.minimum(np.arange(0, n_iv + 100, 100, dtype=np.uint64), np.uint64(n_iv))
    assert offsets[-1] == n_iv and (np.diff(offsets.astype(np.int64)) > 0).all()
    lengths = rng.integers(1, 2**32, size=len(offsets) - 1, dtype=np.uint64).astype(np.uint32)
    return offsets, intervals, lengths
