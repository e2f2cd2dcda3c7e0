"""Inputs and yardsticks shared by tests/test_gunzip_stream_cases.py (the plain-gzip decoder's text on the host, csrc/
inflate_stream.h) and tests/test_gpu_gunzip_stream.py (the same text on the device): single-member gzip streams built with
zlib or bit by bit, a small pure-Python block walker that says where their deflate blocks begin, and the file
tools/inflate_stream_check.cc reads.  The yardstick for the bytes is always Python's zlib."""
import functools
import gzip
import random
import struct
import zlib

import inflate_cases as ic
from deflate_cases import fastq_like, fuzz_text, paf_like  # noqa: F401  (fuzz_text: the GPU test's)
from inflate_cases import Bits, deflate

CHUNKS = (1024, 4096, 32768)


def gz(payload, data=None, flg=0, fields=b"", crc=None, isize=None):
    """one gzip member around a raw deflate `payload`; CRC-32 and ISIZE are `data`'s unless given; `fields`: what FLG announces
    (FEXTRA, FNAME, FCOMMENT), the header's CRC-16 is added where FHCRC is set"""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) & 0xFFFFFFFF if isize is None else isize
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\x03" + fields
    if flg & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + payload + struct.pack("<II", crc, isize)


def zlib_says(blob):
    """the text when zlib takes `blob` as exactly one gzip member with nothing behind it, else None"""
    d = zlib.decompressobj(31)
    try:
        data = d.decompress(blob) + d.flush()
    except zlib.error:
        return None
    return data if d.eof and not d.unused_data else None


# ---- the block walker ---------------------------------------------------------------------------------------------------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical(lens):
    """{symbol: (code, length)} of a canonical Huffman code"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


_FAST = 10


def _table(lens):
    """(one-look table over the next 10 bits: symbol << 4 | length or 0; the longer codes by (reversed code, length); their lengths)"""
    fast, by = [0] * (1 << _FAST), {}
    for s, (c, l) in canonical(lens).items():
        rev = int(format(c, "0%db" % l)[::-1], 2)
        if l <= _FAST:
            for i in range(rev, 1 << _FAST, 1 << l):
                fast[i] = (s << 4) | l
        else:
            by[(rev, l)] = s
    return fast, by, sorted({l for _, l in by})


_FIXED = None


class _Reader:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def take(self, k):
        at = self.pos >> 3
        v = int.from_bytes(self.data[at:at + 4], "little") >> (self.pos & 7)
        self.pos += k
        return v & ((1 << k) - 1)

    def sym(self, tab):
        fast, by, ls = tab
        at = self.pos >> 3
        v = int.from_bytes(self.data[at:at + 4], "little") >> (self.pos & 7)
        e = fast[v & 1023]
        if e:
            self.pos += e & 15
            return e >> 4
        for l in ls:
            s = by.get((v & ((1 << l) - 1), l))
            if s is not None:
                self.pos += l
                return s
        raise ValueError("no code")


@functools.lru_cache(maxsize=None)
def blocks(payload):
    """the blocks of a valid raw deflate stream: [(start bit, BTYPE, BFINAL, text bytes, matches that reach in front of the block)]"""
    global _FIXED
    r, out, pos = _Reader(payload), [], 0
    while True:
        start = r.pos
        final, typ = r.take(1), r.take(2)
        made = crossing = 0
        if typ == 0:
            r.pos = (r.pos + 7) & ~7
            ln = r.take(16)
            r.take(16)
            r.pos += 8 * ln
            made = ln
        else:
            if typ == 1:
                if _FIXED is None:
                    _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30))
                lit, dist = _FIXED
            else:
                hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_CL_ORDER[i]] = r.take(3)
                clt, lens = _table(cl), []
                while len(lens) < hlit + hdist:
                    s = r.sym(clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + r.take(2))
                    elif s == 17:
                        lens += [0] * (3 + r.take(3))
                    else:
                        lens += [0] * (11 + r.take(7))
                lit, dist = _table(lens[:hlit]), _table(lens[hlit:hlit + hdist])
            while True:
                s = r.sym(lit)
                if s < 256:
                    made += 1
                elif s == 256:
                    break
                else:
                    ln = _LEN_BASE[s - 257] + r.take(_LEN_EXTRA[s - 257])
                    ds = r.sym(dist)
                    d = _DIST_BASE[ds] + r.take(_DIST_EXTRA[ds])
                    crossing += d > made
                    made += ln
        out.append((start, typ, final, made, crossing))
        pos += made
        if final:
            return out


def payload_of(blob):
    """the deflate payload of a gzip member made by gz() or gzip.compress (FLG as gz() writes it)"""
    flg, at = blob[3], 10
    if flg & 4:
        at += 2 + struct.unpack("<H", blob[at:at + 2])[0]
    for bit in (8, 16):
        if flg & bit:
            at = blob.index(b"\0", at) + 1
    if flg & 2:
        at += 2
    return blob[at:-8]


def chunks_with_a_start(blob, chunk):
    """chunks k >= 1 of the payload that hold the start of a dynamic, non-final block: what the finder must not miss"""
    return len({start // (8 * chunk) for start, typ, final, _, _ in blocks(payload_of(blob)) if typ == 2 and not final and start >= 8 * chunk})


# ---- hand-made dynamic blocks -------------------------------------------------------------------------------------------
# one code for every hand-made block: literal / length symbols 0-225 in 8 bits and 226-285 in 9, distance symbols 0-1 in 4
# bits and 2-29 in 5 (both complete); the code-length code gives the lengths 0-15 four bits each, and no repeats are used
_LIT_LENS = [8] * 226 + [9] * 60
_DIST_LENS = [4] * 2 + [5] * 28
_LIT, _DIST = canonical(_LIT_LENS), canonical(_DIST_LENS)


class Dyn:
    """a dynamic block written symbol by symbol into a Bits"""

    def __init__(self, bits, final=0):
        self.b = bits
        bits.put(final, 1).put(2, 2).put(29, 5).put(29, 5).put(15, 4)
        for s in _CL_ORDER:
            bits.put(4 if s < 16 else 0, 3)
        for l in _LIT_LENS + _DIST_LENS:
            bits.code(l, 4)

    def lit(self, data):
        for c in data:
            self.b.code(*_LIT[c])
        return self

    def match(self, length, dist):
        ls = max(i for i in range(29) if _LEN_BASE[i] <= length and (i < 28 or length == 258))
        if length == 258:
            ls = 28
        self.b.code(*_LIT[257 + ls]).put(length - _LEN_BASE[ls], _LEN_EXTRA[ls])
        ds = max(i for i in range(30) if _DIST_BASE[i] <= dist)
        self.b.code(*_DIST[ds]).put(dist - _DIST_BASE[ds], _DIST_EXTRA[ds])
        return self

    def end(self):
        self.b.code(*_LIT[256])
        return self.b


def stored(bits, data, final=0):
    bits.put(final, 1).put(0, 2)
    bits.put(0, (-bits.n) % 8)
    bits.put(len(data), 16).put(len(data) ^ 0xFFFF, 16)
    for c in data:
        bits.put(c, 8)
    return bits


def hand_made():
    """One stream, three constructions (far_match_member's idea, in a long stream):
      - a stored block of 40 000 random bytes, then a dynamic block — a span of its own at every chunk size — whose FIRST symbol
        is a match of 258 at distance 32 768: its first source byte is the byte 32 768 in front of the span's first byte;
      - in that span a later match copies those markers; the span then runs on for 40 000 literals, so its first bytes lie
        beyond its last 32 768 and only the bytes step resolves them;
      - a short dynamic block (1 300 bytes of payload: a span of its own at 1 KiB) that begins with a match into the span in
        front of it, and another whose first match copies exactly those bytes: span s + 2 takes what s + 1 took from s."""
    r = random.Random(77)
    b = stored(Bits(), r.randbytes(40000))
    Dyn(b).match(258, 32768).lit(b"xyz").match(258, 261).match(100, 400).lit(r.randbytes(40000)).end()
    Dyn(b).match(100, 20000).lit(r.randbytes(1300)).end()
    Dyn(b).match(100, 1400).lit(r.randbytes(1200)).match(50, 32768).lit(b"end").end()
    b.put(1, 1).put(1, 2).fixed_lit(256)  # the final block: fixed, empty
    pay = b.bytes()
    return pay, zlib.decompress(pay, -15)


def planted_false_start(tail=700):
    """a stored block whose content begins, exactly on the 1 KiB chunk border, with the first 400 bytes of a real multi-block
    deflate stream: more than the acceptance rule reads (a dynamic header is at most 17 + 57 + 316 * 14 bits = 562 bytes, and
    zlib's are a fifth of that), so the finder accepts a header that no block begins with; a real stream follows.  With a
    `tail` of 100 bytes the real stream's first block begins in the same 1 KiB chunk, behind the false start: no span begins
    on it, the chain proves it, and it takes a round of its own"""
    text = paf_like(random.Random(3), 4000)
    real = deflate(text, 6)
    assert blocks(real)[0][1:3] == (2, 0)  # (dynamic, not final: what the finder looks for)
    inner = b"\0" * (1024 - 5) + real[:400] + b"\0" * tail
    pay = stored(Bits(), inner).bytes() + real
    return pay, inner + text


# ---- the streams --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def natural():
    """[(name, gzip member, text)]"""
    out = []
    for what, text in (("overlaps", paf_like(random.Random(1), 12000)), ("reads", fastq_like(random.Random(2), 1500))):
        for lv in (1, 6, 9, 0):
            out.append(("%s, level %d" % (what, lv), gz(deflate(text, lv), text), text))
        for name, st in (("Z_FIXED", zlib.Z_FIXED), ("Z_HUFFMAN_ONLY", zlib.Z_HUFFMAN_ONLY), ("Z_RLE", zlib.Z_RLE)):
            out.append(("%s, %s" % (what, name), gz(deflate(text, 6, st), text), text))
    return out


@functools.lru_cache(maxsize=None)
def valid_cases():
    """[(name, gzip member, text)]: everything the decoder must take"""
    out = list(natural())
    paf = natural()[0][2]
    for name, mode in (("Z_BLOCK", zlib.Z_BLOCK), ("Z_SYNC_FLUSH", zlib.Z_SYNC_FLUSH)):
        out.append(("short spans, %s every 3 000 bytes" % name, gz(deflate(paf, 6, cuts=[(p, mode) for p in range(3000, len(paf), 3000)]), paf), paf))
    pay, text = hand_made()
    out.append(("hand-made: distance 32 768 at a span's first byte, markers copied, a chain of three", gz(pay, text), text))
    pay, text = planted_false_start()
    out.append(("a planted false start", gz(pay, text), text))
    pay, text = planted_false_start(100)
    out.append(("a planted false start in front of a real one in its chunk", gz(pay, text), text))
    small = fastq_like(random.Random(4), 40)
    pay = deflate(small)
    out.append(("FNAME", gz(pay, small, 8, b"reads.fq\0"), small))
    out.append(("FEXTRA", gz(pay, small, 4, struct.pack("<H", 5) + b"ab\x01\x00z"), small))
    out.append(("FCOMMENT", gz(pay, small, 16, b"hello\0"), small))
    out.append(("FHCRC", gz(pay, small, 2), small))
    out.append(("every field", gz(pay, small, 30, struct.pack("<H", 3) + b"abc" + b"n\0" + b"c\0"), small))
    out.append(("gzip.compress", gzip.compress(small), small))
    out.append(("an empty text", gz(deflate(b""), b""), b""))
    out.append(("one byte", gz(deflate(b"A"), b"A"), b"A"))
    return out


def refused_cases():
    """[(name, blob, part of the message or None)]"""
    small = fastq_like(random.Random(4), 40)
    pay = deflate(small)
    good = gz(pay, small)
    out = [
        ("two members", good + good, "left over"),
        ("BGZF", ic.bgzf_of(small * 3), None),
        ("trailing garbage", good + b"\0", None),
        ("reserved FLG bits", gz(pay, small, 0x20), "not a gzip member"),
        ("a truncated trailer", good[:-3], None),
        ("a truncated header", gz(pay, small, 8, b"reads.fq\0")[:15], "not a gzip member"),
        ("shorter than header and trailer", good[:17], "not a gzip member"),
        ("not deflate", b"\x1f\x8b\x07" + good[3:], "not a gzip member"),
        ("a wrong ISIZE", gz(pay, small, isize=len(small) + 1), "ISIZE"),
        ("a wrong CRC", gz(pay, small, crc=zlib.crc32(small) ^ 0x100), "CRC"),
    ]
    for name, blob, cause in ic.not_taken_cases():
        members = ic.walk(blob)
        if len(members) == 2:  # (the case's member and the EOF member)
            payload, crc, isize = members[0]
            out.append(("in a gzip frame: " + name, gz(payload, crc=crc, isize=isize), cause))
    return out


def mutations(n, seed=4711):
    """n gzip members: a natural stream with one bit flipped or one byte replaced"""
    pool = [b for _, b, _ in natural()]
    r = random.Random(seed)
    out = []
    for k in range(n):
        m = bytearray(pool[k % len(pool)])
        # one in four lands in the deflate stream's first bytes, one anywhere in it, one anywhere in the member, and one in the
        # header's ten bytes: in streams of this size only MTIME, XFL, OS and FTEXT are bits that do not matter
        where = r.randrange(4)
        at = r.randrange(10, 10 + 60) if where == 0 else r.randrange(10, len(m) - 8) if where == 1 else r.randrange(len(m)) if where == 2 else r.randrange(10)
        if r.randrange(2):
            m[at] ^= 1 << r.randrange(8)
        else:
            m[at] = (m[at] + r.randrange(1, 256)) & 255
        out.append(bytes(m))
    return out


def write_check_file(path, records):
    """records: (gzip member, chunk, expected text or None: must be refused, may_refuse) -> the file tools/inflate_stream_check.cc reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(records)))
        for blob, chunk, want, may_refuse in records:
            f.write(struct.pack("<QIBQ", len(blob), chunk, 0 if want is None else 2 if may_refuse else 1, len(want) if want is not None else 0))
            f.write(blob)
            if want is not None:
                f.write(want)
