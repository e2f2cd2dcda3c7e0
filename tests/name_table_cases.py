"""What tests/test_name_table_cases.py (CPU) and tests/test_gpu_name_tables.py (GPU) share: the id hash of the device's name
tables (csrc/gpu_text.h: gp_hash) restated, a pool of ids that all home into the LAST 256 slots of every table of at most 2^20
slots, linear probing simulated, the tables' size rules as constants, and builders of overlap texts over a list of ids.
numpy only: nothing here runs the oracle or the engine.

Five kernels find a read by its name in an open-addressing table, all with gp_hash and `(s + 1) & mask`: the device parser's
table of a range (gp_intern, csrc/gpu_paf.hip), its merge table over the engines (gm_intern_kernel), the editors' table
(csrc/edit_table.h) and the report reader's (csrc/gpu_report.hip).  Ids that spread evenly never build a long chain, never
cross a table's last slot on purpose, and never miss inside a chain; the pool's ids do all three."""
import functools

import numpy as np

# ---- the size rules (csrc/gpu_paf.hip: parse_range, GroupRun::merge; gpu_edit.hip / gpu_seq_edit.hip: plan; gpu_report.hip) ------
PARSER_MIN_CAP = 1 << 20   # the parser's table of a range: max(2^20, pow2 >= bytes / 64) slots
WALK_SLOTS = 1025          # gp_intern looks at `probes <= min(mask, 1024)`: at most 1025 slots, then kTableFull
HOME_WINDOW = 256          # the pool: every id's home slot lies in the table's last 256 slots
SEGMENT = 32 * (4 << 20)   # the parse is launched once per 128 MiB of text (csrc/gpu_text.h: kTextChunk * kTextSeg)


def parser_cap(n_bytes):
    """u64 cap = 1 << 20; while (cap < n / 64 && cap < (1 << 31)) cap <<= 1;"""
    cap = PARSER_MIN_CAP
    while cap < n_bytes // 64 and cap < (1 << 31):
        cap <<= 1
    return cap


def parser_holds_comfortably(n_reads, cap):
    """not `(u64)R * 2 > cap && R > 1024`: the text is taken"""
    return not (n_reads * 2 > cap and n_reads > 1024)


def pow2_cap(n):
    """cap = 1024; while (cap < 2 * n) cap <<= 1 — the merge table (n = M, the sum of the ranges' read counts), the editors'
    table (n = R reads) and the report reader's (n = lines)"""
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


# ---- gp_hash -----------------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
_SEED, _GOLD, _PRIME, _MIX = 0xcbf29ce484222325, 0x9E3779B97F4A7C15, 0x100000001b3, 0xbf58476d1ce4e5b9


def gp_hash(ids):
    """gp_hash over the rows of an (N, L) uint8 array -> uint64[N] (uint64 arithmetic wraps: everything is mod 2^64)"""
    ids = np.asarray(ids, np.uint8)
    n, length = ids.shape
    h = np.full(n, _SEED ^ ((length * _GOLD) & _M64), np.uint64)
    for k in range(length):
        h = (h ^ ids[:, k].astype(np.uint64)) * np.uint64(_PRIME)
    h ^= h >> np.uint64(29)
    h *= np.uint64(_MIX)
    return h ^ (h >> np.uint64(32))


def gp_hash_scalar(name):
    """the same over one `bytes`, in Python integers"""
    h = _SEED ^ ((len(name) * _GOLD) & _M64)
    for b in name:
        h = ((h ^ b) * _PRIME) & _M64
    h ^= h >> 29
    h = (h * _MIX) & _M64
    return h ^ (h >> 32)


def homes(ids, cap):
    """the home slots of ids (a list of bytes of any lengths) in a table of `cap` slots -> int64[len(ids)]"""
    out = np.zeros(len(ids), np.int64)
    by_len = {}
    for i, x in enumerate(ids):
        by_len.setdefault(len(x), []).append(i)
    for length, idx in by_len.items():
        rows = np.frombuffer(b"".join(ids[i] for i in idx), np.uint8).reshape(len(idx), length)
        out[idx] = (gp_hash(rows) & np.uint64(cap - 1)).astype(np.int64)
    return out


# ---- the pool ----------------------------------------------------------------------------------------------------------------------
ALPHABET = b"abcdefghijklmnopqrstuvwxyz234567"  # 32 letters; no tab, space, '"' or CR
_LETTERS = np.frombuffer(ALPHABET, np.uint8)
_BATCH = 1 << 20


def _candidates(first, count):
    """candidates first .. first + count - 1 of the enumeration: 'p' and the seven base-32 digits of the number, high digit first"""
    k = np.arange(first, first + count, dtype=np.int64)
    rows = np.empty((count, 8), np.uint8)
    rows[:, 0] = ord("p")
    for d in range(7):
        rows[:, 1 + d] = _LETTERS[(k >> (5 * (6 - d))) & 31]
    return rows


_pool_rows, _pool_next = [], [0]


def pool(n):
    """The first n ids (bytes of 8) of the enumeration whose hash has its low 20 bits >= 2^20 - 256.  Such an id's home lies in
    the last 256 slots of EVERY table of 2^b slots, 10 <= b <= 20: when the low 20 bits are >= 2^20 - 256, bits 8..19 are all
    ones, so the low b bits are >= 2^b - 256.  About one candidate in 4096 is taken; the pool grows as it is asked for and
    is kept for the process."""
    while len(_pool_rows) < n:
        rows = _candidates(_pool_next[0], _BATCH)
        _pool_next[0] += _BATCH
        low = gp_hash(rows) & np.uint64(PARSER_MIN_CAP - 1)
        for r in rows[low >= np.uint64(PARSER_MIN_CAP - HOME_WINDOW)]:
            _pool_rows.append(r.tobytes())
    return _pool_rows[:n]


# ---- linear probing ----------------------------------------------------------------------------------------------------------------
def occupied(ids, cap, order=None):
    """ids inserted one by one, in `order` (indices into ids; default: as listed), each walking from its home slot to the
    first empty one -> (mask bool[cap] of the occupied slots, examined int64[len(ids)]: the slots id i looked at, the one it
    took included).  The mask does not depend on the order; the walks do."""
    home = homes(ids, cap)
    nxt = list(range(cap))  # nxt[s]: a slot at or behind s (cyclically) that may be empty; an empty slot names itself

    def first_free(s):
        path = []
        while nxt[s] != s:
            path.append(s)
            s = nxt[s]
        for q in path:
            nxt[q] = s
        return s

    assert len(ids) < cap
    examined = np.zeros(len(ids), np.int64)
    mask = np.zeros(cap, bool)
    for i in (range(len(ids)) if order is None else order):
        h = int(home[i])
        s = first_free(h)
        mask[s] = True
        nxt[s] = (s + 1) % cap
        examined[i] = (s - h) % cap + 1
    return mask, examined


def occupied_mask(home, cap):
    """the occupied slots of a table that holds ids with these home slots (fewer than cap), without walking: slot s is taken
    when an id homes there or one spills over from s - 1; the spill is a queue, o[s] = max(0, o[s - 1] + c[s] - 1), that is
    P[s] - min(P[..s]) over the running sum P of c - 1, taken twice round the table so that it wraps"""
    c = np.bincount(np.asarray(home, np.int64), minlength=cap).astype(np.int64)
    assert c.sum() < cap
    d = np.concatenate([c, c]) - 1
    p = np.cumsum(d)
    o = p - np.minimum(np.minimum.accumulate(p), 0)  # the spill behind slot s (the queue starts empty: min over the empty prefix is 0)
    before = np.concatenate([[0], o[:-1]])
    return ((before + np.concatenate([c, c])) >= 1)[cap:]


def clusters(mask):
    """the runs of occupied slots of a table, cyclically -> [(first slot, length)], a run across the last slot listed once"""
    cap = len(mask)
    if mask.all():
        return [(0, cap)]
    z = int(np.nonzero(~mask)[0][0])
    m = np.roll(mask, -z)  # m[0] is empty
    edge = np.diff(m.astype(np.int8))
    starts, ends = np.nonzero(edge == 1)[0] + 1, np.nonzero(edge == -1)[0] + 1
    if len(ends) < len(starts):
        ends = np.append(ends, cap)
    return [((int(s) + z) % cap, int(e - s)) for s, e in zip(starts, ends)]


def longest_cluster(mask):
    return max([n for _, n in clusters(mask)] or [0])


def wraps(mask):
    """a cluster holds the table's last slot and its first"""
    return bool(mask[0] and mask[-1])


# ---- texts -------------------------------------------------------------------------------------------------------------------------
def length_of(i):
    """the length of the i-th id of a text, the same wherever it is named"""
    return 9000 + 7 * (i % 100)


def overlap_line(ids, i, m4=False):
    """record i over K = len(ids) ids: it pairs ids[i % K] with ids[(7 i + 1) % K].  PAF (a la sa ea strand b lb sb eb + three
    columns) or M4 (a b err shared strand sa ea la strand sb eb lb)."""
    K = len(ids)
    a, b = i % K, (7 * i + 1) % K
    sa, sb = (37 * i) % 8000, (53 * i) % 8000
    ea, eb = sa + 1 + (13 * i) % 900, sb + 1 + (17 * i) % 900
    if m4:
        return b"%s %s 0.1 2 0 %d %d %d %d %d %d %d\n" % (ids[a], ids[b], sa, ea, length_of(a), i & 1, sb, eb, length_of(b))
    return b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\n" % (ids[a], length_of(a), sa, ea, b"+-"[i & 1:(i & 1) + 1], ids[b], length_of(b),
                                                                     sb, eb, ea - sa, eb - sb)


def overlap_lines(ids, m4=False, rounds=2):
    """records 0 .. rounds * K - 1: every id is named `rounds` times as the first read, and looked up again where it stands
    (finding an id walks its chain as inserting it did)"""
    return [overlap_line(ids, i, m4) for i in range(rounds * len(ids))]


def overlap_text(ids, m4=False, rounds=2):
    return b"".join(overlap_lines(ids, m4, rounds))


def distinct_ids(n):
    """n plain names, r0 r1 .. in hexadecimal"""
    return [b"r%x" % i for i in range(n)]


def _lines_of(fmt, *columns):
    """one line per row of the precomputed columns (numpy arrays), formatted whole and joined once"""
    return "".join(map(fmt.__mod__, zip(*(c.tolist() for c in columns)))).encode()


def distinct_text(n_ids):
    """a PAF text that names r0 .. r(n_ids - 1), each on ONE record side: line j pairs r(2j) with r(2j + 1), and where n_ids is
    odd a last line pairs the last id with r0"""
    j = np.arange((n_ids + 1) // 2)
    b = 2 * j + 1
    b[b >= n_ids] = 0
    sa, sb = (37 * j) % 8000, (53 * j) % 8000
    return _lines_of("r%x\t9000\t%d\t%d\t+\tr%x\t9000\t%d\t%d\n", 2 * j, sa, sa + 1 + (13 * j) % 900, b, sb, sb + 1 + (17 * j) % 900)


def read_to_reference(n_lines):
    """the everyday read-to-reference PAF: one target, a new query id on every line"""
    j = np.arange(n_lines)
    sa, sb = (37 * j) % 8000, (7919 * j) % 4000000
    return _lines_of("q%x\t9000\t%d\t%d\t+\tref\t5000000\t%d\t%d\n", j, sa, sa + 1 + (13 * j) % 900, sb, sb + 1 + (17 * j) % 900)


# ---- the device parser's cases -------------------------------------------------------------------------------------------------------
def chain_ids(n_pool=900, n_plain=50):
    """case (a): a chain of n_pool slots across the table's end, and a few plain ids beside it"""
    return pool(n_pool) + [b"plain%d" % i for i in range(n_plain)]


FILLER_ID = b"filler"


def walk_case(walk, m4=False):
    """A text whose LAST new id looks at exactly `walk` slots of the parser's table, whatever order the device's atomics
    produce: the first 128 MiB — one launch of the parse — name K pool ids, which fill the block [m, m + K), and
    FILLER_ID on long lines up to the segment's end; behind it, in the next launch, comes one more pool id X (a later one of
    the pool) whose home is h >= m.  Every slot from h to the block's end is taken by then, so X looks at m + K - h + 1 slots; K is chosen so that this
    is `walk`.  -> (text, K, X)"""
    cap = parser_cap(SEGMENT + 64)  # 2^22 slots: the text has more than 2^21 * 64 bytes (asserted below)
    P, n = [], 4 * (walk + HOME_WINDOW + 1)
    while len(P) < walk + HOME_WINDOW + 1:  # the pool's ids that home into the last 256 of 2^22 slots: one in four
        P = [x for x, h in zip(pool(n), homes(pool(n), cap)) if h >= cap - HOME_WINDOW]
        n += 512
    hp = homes(P, cap)
    for K, j in ((K, j) for K in range(walk - 1, walk + HOME_WINDOW) for j in range(K, len(P))):  # (m <= h < m + 256: K - 254 <= the walk <= K + 1)
        m, x, h = int(hp[:K].min()), P[j], int(hp[j])
        if h >= m and m + K - h + 1 == walk:
            break
    else:
        raise AssertionError("no K gives a walk of %d slots" % walk)
    head = overlap_text(P[:K] + [FILLER_ID], m4)
    if m4:
        fill = b"%s %s 0.1 2 0 5 900 9000 0 7 800 9000 %s\n" % (FILLER_ID, FILLER_ID, b"x" * 8000)
        tail = b"%s %s 0.1 2 0 11 700 4000 1 13 600 %d\n" % (x, P[0], length_of(0))
    else:
        fill = b"%s\t9000\t5\t900\t+\t%s\t9000\t7\t800\ttg:Z:%s\n" % (FILLER_ID, FILLER_ID, b"x" * 8000)
        tail = b"%s\t4000\t11\t700\t-\t%s\t%d\t13\t600\n" % (x, P[0], length_of(0))
    n_fill = (SEGMENT - len(head)) // len(fill) + 1  # the last filler line ends behind the segment: X's line starts in the next one
    text = head + fill * n_fill + tail * 2
    assert len(head) + (n_fill - 1) * len(fill) < SEGMENT <= len(head) + n_fill * len(fill)
    assert parser_cap(len(text)) == cap
    ids = P[:K] + [FILLER_ID, x]
    mask, examined = occupied(ids, cap)  # (x last; the order of the others does not matter to x)
    assert int(examined[-1]) == walk, "the filler id got in the way"
    return text, K, x


# ---- the merge table's case ----------------------------------------------------------------------------------------------------------
RANGE_BYTES = 32768  # YACRD_TEST_RANGE_BYTES of the child process: the ranges are cut every 32 KiB


def range_cuts(n_bytes, n_engines, grain=RANGE_BYTES):
    """GroupRun::cut_ranges: whole grains, the same number for every engine -> [B[0] .. B[N]]"""
    chunks = (n_bytes + grain - 1) // grain
    per = (chunks + n_engines - 1) // n_engines
    return [min(n_bytes, d * per * grain) for d in range(n_engines + 1)]


def ids_per_range(text, cuts, m4=False):
    """the ids each range sees: a line belongs to the range it STARTS in -> [set of ids per range]"""
    delim, ib = (b" ", 1) if m4 else (b"\t", 5)
    seen = [set() for _ in cuts[:-1]]
    pos = 0
    for line in text.split(b"\n"):
        if line:
            d = max(k for k in range(len(cuts) - 1) if cuts[k] <= pos)
            f = line.split(delim)
            seen[d].update((f[0], f[ib]))
        pos += len(line) + 1
    return seen


def merge_text(n_engines, ids, late=()):
    """exactly n_engines * 32 KiB of PAF in which every 32 KiB range names all of `ids` (record i pairs ids[i % K] with
    ids[(7 i + 1) % K]: K lines in a row name every id, and a range holds more than two such runs); `late`: ids that only the
    LAST range names, on lines in front of the last one.  The last line carries a tag as long as it takes."""
    total = n_engines * RANGE_BYTES
    late_lines = overlap_lines(list(late) + list(ids[:1])) if late else []
    size = sum(map(len, late_lines))
    lines, i = [], 0
    while size < total - 400:
        lines.append(overlap_line(ids, i))
        size += len(lines[-1])
        i += 1
    last = overlap_line(ids, i)[:-1] + b"\ttg:Z:"
    pad = total - size - len(last) - 1
    assert pad >= 0
    text = b"".join(lines + late_lines) + last + b"y" * pad + b"\n"
    assert len(text) == total
    return text


# ---- the editors' and the reader's tables ----------------------------------------------------------------------------------------------
PLAIN_HELD = [b"plain%d" % i for i in range(20)]        # plain ids the tables hold
PLAIN_ABSENT = [b"plain%d" % i for i in range(20, 40)]  # and plain ids they do not


def type_of(i):
    return (5 * i + 1) % 3  # NotBad, Chimeric and NotCovered mixed


@functools.lru_cache(maxsize=None)
def close_ids():
    """What separates an id from its neighbours in a chain, for the table of 1024 slots: (a, b, c) — pool ids a and b that
    differ only in their LAST byte, and c, which differs from both in that byte only and homes into the last 256 of 1024
    slots (c is for the text alone); (p, px, py) — a pool id, and two of its extensions by two letters that home there as well
    (p and px are table entries, p a proper prefix of px; py is for the text alone)."""
    P = pool(2200)
    by_stem = {}
    pair = None
    for x in P:
        if x[:7] in by_stem:
            pair = (by_stem[x[:7]], x)
            break
        by_stem[x[:7]] = x
    assert pair is not None, "no two pool ids share their first seven bytes"
    a, b = pair
    sib = [a[:7] + bytes([ch]) for ch in ALPHABET if bytes([ch]) not in (a[7:], b[7:])]
    sib = [s for s, h in zip(sib, homes(sib, 1024)) if h >= 768]
    p = P[0]
    ext = [p + bytes([u, v]) for u in ALPHABET for v in ALPHABET]
    ext = [e for e, h in zip(ext, homes(ext, 1024)) if h >= 768]
    assert sib and len(ext) >= 2
    return (a, b, sib[0]), (p, ext[0], ext[1])


def small_table():
    """-> (names, types): 400 pool ids — a and b of close_ids among them, the pool's first ones beside them —, px and twenty
    plain ids; 1024 slots"""
    (a, b, _), (p, px, _) = close_ids()
    names = [a, b] + [x for x in pool(400) if x not in (a, b)][:398] + [px] + PLAIN_HELD
    assert p in names and len(set(names)) == 421 and pow2_cap(len(names)) == 1024
    return names, [type_of(i) for i in range(len(names))]


def large_table():
    """-> (names, types): the pool's first 1400 ids and twenty plain ones; 4096 slots, a chain of about 1380 slots across the end"""
    names = pool(1400) + PLAIN_HELD
    assert pow2_cap(len(names)) == 4096
    return names, [type_of(i) for i in range(len(names))]


def absent_pool_ids(names, n=300):
    """the pool's next n ids behind those a table holds: they home inside its chain, so a correct miss walks to the chain's far
    end, across the wrap"""
    held = set(names)
    return [x for x in pool(len(names) + n + 2) if x not in held][:n]


def lookup_ids(names, small):
    """what a text names against a table: its ids (pool and plain), pool ids it does not hold, plain ids it does not hold, and
    for the small table the close ids -> list of bytes"""
    out = list(names) + absent_pool_ids(names) + PLAIN_ABSENT
    if small:
        (_, _, c), (_, _, py) = close_ids()
        out += [c, py]
    return out


def report_rows(ids, n_dup):
    """a .yacrd report over ids, and n_dup of them again further down with other values: the first position is kept, the last
    values win -> bytes"""
    K = len(ids)
    rows = [b"%s\t%s\t%d\t%s\n" % ((b"NotBad", b"Chimeric", b"NotCovered")[type_of(i)], x, 1000 + i,
                                  b"" if i % 3 == 0 else b"%d,%d,%d;7,900,907" % (i % 90 + 1, 10, 11 + i % 90)) for i, x in enumerate(ids)]
    for k in range(n_dup):
        i = (11 * k + 3) % K
        rows.append(b"NotBad\t%s\t%d\t%s\n" % (ids[i], 5000 + k, b"" if k % 4 == 0 else b"3,%d,%d" % (k, k + 3)))
    return b"".join(rows)
