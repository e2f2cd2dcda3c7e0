"""Inputs and yardsticks shared by tests/test_inflate_cases.py (the decoder's text on the host) and tests/test_gpu_inflate.py
(the same text on the device): BGZF streams built here with zlib or bit by bit, what Python's zlib makes of them, and the
file tools/inflate_check.cc reads."""
import gzip
import random
import struct
import zlib

from deflate_cases import BLOCK, EOF_MEMBER, fastq_like, fuzz_text, paf_like

BC = b"BC\x02\x00"


def frame(payload, data=None, extra_front=b"", crc=None, isize=None, flg=4, after_header=b""):
    """One member around a raw deflate `payload`; CRC-32 and ISIZE are `data`'s unless given."""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    xlen = len(extra_front) + 6
    size = 12 + xlen + len(after_header) + len(payload) + 8
    assert size <= 65536, size
    return (b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_front + BC + struct.pack("<H", size - 1) +
            after_header + payload + struct.pack("<II", crc, isize))


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=()):
    """raw deflate of `data`; `cuts`: (position, flush mode) pairs that end a block there"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out, at = [], 0
    for pos, mode in cuts:
        out.append(c.compress(data[at:pos]) + c.flush(mode))
        at = pos
    out.append(c.compress(data[at:]) + c.flush())
    return b"".join(out)


def member(data, *a, **k):
    return frame(deflate(data, *a, **k), data)


class Bits:
    """a deflate bit stream written by hand: fields least significant bit first, Huffman codes most significant first"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n)
        self.acc |= v << self.n
        self.n += n
        return self

    def code(self, c, n):
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)
        return self

    def fixed_lit(self, s):
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        if s < 280:
            return self.code(s - 256, 7)
        return self.code(0xC0 + s - 280, 8)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def far_match_member():
    """fixed Huffman: 32 768 literals, then a match of 258 at distance 32 768 (zlib never looks that far): it reaches byte 0"""
    lit = random.Random(5).randbytes(32768)
    b = Bits().put(1, 1).put(1, 2)
    for c in lit:
        b.fixed_lit(c)
    b.fixed_lit(285).code(29, 5).put(32768 - 24577, 13).fixed_lit(256)
    return frame(b.bytes(), lit + lit[:258]), lit + lit[:258]


def valid_cases():
    """[(name, BGZF stream, its text)]"""
    r = random.Random(20250101)
    reads = fastq_like(r, 260)[:BLOCK]
    paf = paf_like(r, 700)[:BLOCK]
    noise = r.randbytes(65505)
    runs = b"".join(bytes([r.randrange(256)]) * r.randrange(200, 900) for _ in range(60))
    out = []

    def one(name, m, text):
        out.append((name, m + EOF_MEMBER, text))

    one("level 0 (stored)", member(reads[:50000], 0), reads[:50000])
    one("Z_FIXED", member(reads[:30000], 6, zlib.Z_FIXED), reads[:30000])
    for lv in (1, 6, 9):
        one("level %d" % lv, member(reads, lv), reads)
        one("level %d, overlaps" % lv, member(paf, lv), paf)
    one("Z_HUFFMAN_ONLY", member(reads[:40000], 6, zlib.Z_HUFFMAN_ONLY), reads[:40000])
    one("Z_RLE", member(runs, 6, zlib.Z_RLE), runs)
    one("several blocks", member(reads, 6, cuts=[(1000, zlib.Z_FULL_FLUSH), (1001, zlib.Z_SYNC_FLUSH), (30000, zlib.Z_SYNC_FLUSH),
                                                 (30000, zlib.Z_FULL_FLUSH), (60000, zlib.Z_FULL_FLUSH)]), reads)
    m, text = far_match_member()
    one("distance 32 768, reaching byte 0", m, text)
    big = (reads * 2)[:65536]
    for n in (0, 1, 65279, 65280, 65536):
        one("ISIZE %d" % n, member(big[:n]), big[:n])
    m = frame(b"\x01" + struct.pack("<HH", len(noise), len(noise) ^ 0xFFFF) + noise, noise)  # one stored block
    assert len(m) == 65536
    one("incompressible, 65 536-byte member", m, noise)
    a, b = member(reads[:700]), member(paf[:900], 1)
    out.append(("EOF members everywhere", EOF_MEMBER + a + EOF_MEMBER + EOF_MEMBER + b + EOF_MEMBER, reads[:700] + paf[:900]))
    out.append(("no EOF member", a + b, reads[:700] + paf[:900]))
    out.append(("a subfield in front of BC", frame(deflate(paf[:5000]), paf[:5000], extra_front=b"XY\x03\x00abc") + EOF_MEMBER, paf[:5000]))
    out.append(("empty input", b"", b""))
    out.append(("EOF only", EOF_MEMBER, b""))
    return out


def encoder_cases(seeds):
    """[(name, stream, text)]: the project's own encoder over fuzz_text"""
    from yacrd_amd import host
    return [("encoder, seed %d" % s, host.bgzf_encode_host(fuzz_text(s)), fuzz_text(s)) for s in seeds]


def _dyn(hlit=0, hdist=0, cl=()):
    """a last dynamic block's header up to the code-length code's lengths (in the order they are sent)"""
    b = Bits().put(1, 1).put(2, 2).put(hlit, 5).put(hdist, 5).put(len(cl) - 4, 4)
    for v in cl:
        b.put(v, 3)
    return b


def not_taken_cases():
    """[(name, stream, cause)]: `cause` is part of the host decoder's message"""
    r = random.Random(7)
    text = fastq_like(r, 20)
    pay = deflate(text)
    out = []

    def one(name, m, cause):
        out.append((name, m + EOF_MEMBER, cause))

    one("payload ends early", frame(pay[:-1], text), "ends early")
    one("payload ends early, in a stored block", frame(b"\x01\x05\x00\xfa\xffabc", b"abcde"), "ends early")
    one("payload ends at once", frame(b"", b""), "ends early")
    one("payload has bytes left over", frame(pay + b"\0", text), "left over")
    one("block type 3", frame(b"\x07", b""), "block type 3")
    one("LEN / NLEN mismatch", frame(b"\x01\x05\x00\xfb\xffabcde", b"abcde"), "LEN / NLEN")
    one("over-subscribed code lengths", frame(_dyn(cl=(1, 1, 1, 1)).bytes() + b"\0\0", b""), "over-subscribed")
    one("incomplete code lengths", frame(_dyn(cl=(2, 0, 0, 2)).bytes() + b"\0\0", b""), "incomplete")
    # the code-length code: 0 -> '0', 16 -> '1'; the first length sent is symbol 16
    one("repeat code 16 with nothing in front", frame(_dyn(cl=(1, 0, 0, 1)).put(1, 1).put(0, 2).bytes() + b"\0\0", b""), "repeat")
    one("HLIT beyond 286", frame(_dyn(hlit=30, cl=(1, 0, 0, 1)).bytes() + b"\0\0", b""), "HLIT / HDIST")
    one("HDIST beyond 30", frame(_dyn(hdist=30, cl=(1, 0, 0, 1)).bytes() + b"\0\0", b""), "HLIT / HDIST")
    one("length symbol 286", frame(Bits().put(1, 1).put(1, 2).fixed_lit(97).fixed_lit(286).code(0, 5).fixed_lit(256).bytes(), b"aaaa"), "invalid symbol")
    one("distance symbol 30", frame(Bits().put(1, 1).put(1, 2).fixed_lit(97).fixed_lit(257).code(30, 5).fixed_lit(256).bytes(), b"aaaa"), "invalid symbol")
    one("a distance beyond the produced bytes", frame(Bits().put(1, 1).put(1, 2).fixed_lit(97).fixed_lit(257).code(1, 5).fixed_lit(256).bytes(), b"aaaa"),
        "distance beyond")
    one("output beyond ISIZE", frame(pay, text, isize=len(text) - 1), "ISIZE")
    one("output short of ISIZE", frame(pay, text, isize=len(text) + 1), "ISIZE")
    one("output beyond ISIZE, by a match", frame(deflate(b"a" * 600), b"a" * 600, isize=300), "ISIZE")
    one("CRC mismatch", frame(pay, text, crc=zlib.crc32(text) ^ 0x100), "CRC")
    good = member(text)
    out.append(("a refused member behind good ones", good + good + frame(pay, text, crc=1) + good + EOF_MEMBER, "member 2 not taken: CRC"))
    return out


def not_bgzf_cases():
    """[(name, stream)]: framings the member walk does not take"""
    r = random.Random(8)
    text = fastq_like(r, 20)
    pay, good = deflate(text), member(text)
    plain = gzip.compress(text, 1)
    hdr_no_bc = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"XY\x02\x00\x00\x00"
    return [
        ("plain gzip", plain),
        ("plain gzip behind a member", good + plain),
        ("FNAME set", frame(pay, text, flg=4 | 8, after_header=b"reads.fq\0") + EOF_MEMBER),
        ("FCOMMENT set", frame(pay, text, flg=4 | 16, after_header=b"hello\0") + EOF_MEMBER),
        ("FHCRC set", frame(pay, text, flg=4 | 2, after_header=b"\x12\x34") + EOF_MEMBER),
        ("BSIZE beyond the input", good + good[:-3]),
        ("bytes after the last member", good + EOF_MEMBER + b"\0"),
        ("a header cut short", good + EOF_MEMBER[:11]),
        ("no BC subfield", hdr_no_bc + pay + struct.pack("<II", zlib.crc32(text), len(text))),
        ("two BC subfields", frame(pay, text, extra_front=BC + b"\x10\x00") + EOF_MEMBER),
        ("a subfield beyond XLEN", frame(pay, text, extra_front=b"XY\x40\x00a") + EOF_MEMBER),
        ("BSIZE smaller than the frame", good[:16] + struct.pack("<H", 20) + good[18:]),
        ("not deflate", b"\x1f\x8b\x07\x04" + good[4:]),
    ]


def walk(blob):
    """the member walk's rules, restated: [(payload, crc, isize)] or None (not BGZF)"""
    out, at = [], 0
    while at < len(blob):
        h = blob[at:]
        if len(h) < 12 or h[:4] != b"\x1f\x8b\x08\x04":
            return None
        end = 12 + struct.unpack("<H", h[10:12])[0]
        if end > len(h):
            return None
        q, bsize = 12, None
        while q + 4 <= end:
            slen = struct.unpack("<H", h[q + 2:q + 4])[0]
            if slen > end - (q + 4):
                return None
            if h[q:q + 2] == b"BC":
                if slen != 2 or bsize is not None:
                    return None
                bsize = struct.unpack("<H", h[q + 4:q + 6])[0]
            q += 4 + slen
        if q != end or bsize is None:
            return None
        size = bsize + 1
        if size < end + 8 or size > len(h):
            return None
        crc, isize = struct.unpack("<II", h[size - 8:size])
        if isize > 65536:
            return None
        out.append((h[end:size - 8], crc, isize))
        at += size
    return out


def zlib_says(blob):
    """the text when zlib takes every member of `blob` exactly (its payload whole, CRC-32 and ISIZE matching), else None"""
    members = walk(blob)
    if members is None:
        return None
    out = []
    for payload, crc, isize in members:
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(payload) + d.flush()
        except zlib.error:
            return None
        if not d.eof or d.unused_data or len(data) != isize or zlib.crc32(data) != crc:
            return None
        out.append(data)
    return b"".join(out)


def mutation_pool():
    r = random.Random(99)
    reads, paf = fastq_like(r, 12), paf_like(r, 30)
    runs = b"".join(bytes([r.randrange(256)]) * r.randrange(1, 400) for _ in range(12))
    return [member(reads, 6), member(reads, 1), member(paf, 9), member(reads[:900], 6, zlib.Z_FIXED), member(paf[:700], 0),
            member(reads[:1500], 6, zlib.Z_HUFFMAN_ONLY), member(runs, 6, zlib.Z_RLE), member(r.randbytes(300), 6),
            member(paf, 6, cuts=[(500, zlib.Z_FULL_FLUSH), (1500, zlib.Z_SYNC_FLUSH)]), member(b"ACGT" * 700, 6),
            frame(deflate(reads[:800]), reads[:800], extra_front=b"XY\x01\x00z")]


def mutations(n, seed=12345):
    """n streams: a member of the pool (an EOF member behind it) with one bit flipped or one byte replaced"""
    pool = mutation_pool()
    r = random.Random(seed)
    out = []
    for k in range(n):
        m = bytearray(pool[k % len(pool)])
        # three in four land in the deflate stream's first bytes or anywhere in it; the rest anywhere in the member
        where = r.randrange(3)
        at = r.randrange(18, min(len(m), 18 + 60)) if where == 0 else r.randrange(18, len(m) - 8) if where == 1 else r.randrange(len(m))
        if r.randrange(2):
            m[at] ^= 1 << r.randrange(8)
        else:
            m[at] = (m[at] + r.randrange(1, 256)) & 255
        out.append(bytes(m) + EOF_MEMBER)
    return out


def write_check_file(path, records):
    """records: (stream, expected text or None: must be refused, may_refuse) -> the file tools/inflate_check.cc reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(records)))
        for blob, want, may_refuse in records:
            f.write(struct.pack("<QBQ", len(blob), 0 if want is None else 2 if may_refuse else 1, len(want) if want is not None else 0))
            f.write(blob)
            if want is not None:
                f.write(want)


def stored_member(data):
    """one stored block, by hand (zlib cuts stored blocks by its output space)"""
    return frame(b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + bytes(data), data)


def bgzf_of(text, chunk=BLOCK, level=6, stored=False):
    """`text` as a BGZF stream of zlib's (or stored) members of `chunk` bytes, the EOF member last"""
    text = bytes(text)
    make = stored_member if stored else (lambda d: member(d, level))
    return b"".join(make(text[i:i + chunk]) for i in range(0, len(text), chunk)) + EOF_MEMBER
