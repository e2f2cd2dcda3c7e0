"""Inputs and yardsticks shared by tests/test_byte_sink.py and tests/test_gpu_deflate.py (device deflate, BGZF)."""
import random
import struct
import zlib

BLOCK = 65280
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def walk_bgzf(blob):
    """[(member bytes, inflated payload)] of a BGZF stream; every header field, BSIZE, CRC-32 and ISIZE are checked."""
    out, at = [], 0
    while at < len(blob):
        h = blob[at:at + 18]
        assert len(h) == 18 and h[:4] == b"\x1f\x8b\x08\x04", "member header at %d" % at
        assert h[4:10] == b"\0\0\0\0\0\xff" and h[10:16] == b"\x06\0BC\x02\0", "MTIME / XFL / OS / the BC subfield at %d" % at
        size = struct.unpack("<H", h[16:18])[0] + 1
        assert size <= 65536 and at + size <= len(blob)
        m = blob[at:at + size]
        d = zlib.decompressobj(-15)
        data = d.decompress(m[18:-8]) + d.flush()
        assert d.eof and d.unused_data == b"", "the deflate stream fills the member exactly"
        crc, isize = struct.unpack("<II", m[-8:])
        assert crc == zlib.crc32(data) and isize == len(data)
        out.append((m, data))
        at += size
    return out


def huffman_only_size(d):
    """H(d): per 65 280-byte block, zlib raw deflate with Z_HUFFMAN_ONLY, plus the 26 bytes of a member's frame."""
    total = 0
    for i in range(0, len(d), BLOCK):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        total += len(c.compress(d[i:i + BLOCK]) + c.flush()) + 26
    return total


def level1_size(d):
    """L(d): the same at level 1, default strategy."""
    total = 0
    for i in range(0, len(d), BLOCK):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(d[i:i + BLOCK]) + c.flush()) + 26
    return total


def fastq_like(r, n_reads, const_quality=False):
    out = []
    for i in range(n_reads):
        ln = r.randrange(50, 400)
        seq = bytes(r.choice(b"ACGT") for _ in range(ln))
        qual = b"?" * ln if const_quality else bytes(r.choice(b"!#%+5?IJ") for _ in range(ln))
        out.append(b"@read%07d ch=%d\n" % (i, r.randrange(512)) + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


def paf_like(r, n_lines):
    out = []
    for _ in range(n_lines):
        a, b = r.randrange(500), r.randrange(500)
        la, lb = 8000 + a * 13, 8000 + b * 13
        s = r.randrange(la // 2)
        out.append(b"r%09d\t%d\t%d\t%d\t%s\tr%09d\t%d\t%d\t%d\t%d\t%d\t255\ttp:A:S\n" % (
            a, la, s, s + la // 3, r.choice([b"+", b"-"]), b, lb, s // 2, s // 2 + lb // 3, la // 4, la // 3))
    return b"".join(out)


def fuzz_text(seed):
    """A text of mixed structure; lengths gather around the block boundaries and around multiples of them."""
    r = random.Random(seed)
    kind = seed % 6
    edge = r.choice([0, 1, 2, 3, 5, 17, 255, 256, 1023, 1024, 4096, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1,
                     4 * BLOCK - 1, 4 * BLOCK, 4 * BLOCK + 1])
    n = max(0, edge + r.choice([0, 0, -1, 1, r.randrange(-300, 300)])) if seed % 3 else r.randrange(1, 3 * BLOCK)
    if kind == 0:
        d = fastq_like(r, n // 300 + 2)
    elif kind == 1:
        d = paf_like(r, n // 90 + 2)
    elif kind == 2:  # runs
        d = b"".join(bytes([r.randrange(256)]) * r.randrange(1, 700) for _ in range(n // 300 + 2))
    elif kind == 3:  # noise
        d = r.randbytes(n + 1)
    elif kind == 4:  # a small alphabet
        d = bytes(r.choice(b"ACGTN\n") for _ in range(n + 1))
    else:  # pieces of everything
        parts = []
        while sum(map(len, parts)) < n + 1:
            parts.append(r.choice([fastq_like(r, 3), paf_like(r, 4), r.randbytes(r.randrange(1, 500)), bytes(r.randrange(1, 3000))]))
        d = b"".join(parts)
    return d[:n]
