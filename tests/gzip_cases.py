"""tests/gzip_cases.py — plain gzip files designed for the chunked inflate of gap2seq_amd/csrc/gzip_chunks.h (compiled for
the host: gzip_inflate(..., device=-2); on the device: the kernels of gzip_inflate.hip), and a model of what its finder
must find.  What zlib can be asked for comes from it; what it will not emit on request (a distance of 32 768, a block
start at a chosen byte, a stored block that looks like a block start) is written bit by bit with the writer of
inflate_cases.py.  The oracle of every case is Python's zlib.decompress of the same bytes; self_check() runs it over every
designed stream, so that a wrong design fails where it is written.

A designed stream uses one dynamic code throughout (UNIVERSAL: every literal in 9 bits, end-of-block and the lengths in 5
and 6, the distances in 4 and 5 — complete, so the acceptance test takes it) and knows the bit at which each of its
non-final dynamic blocks begins: Design.starts.  model_found(design, chunk) is then what the finder must report when the
acceptance test has no false positive: the first such start inside every chunk behind the first."""
import functools
import gzip
import io
import random
import struct
import zlib

import inflate_cases as IC

LIT_LENS = [9] * 256 + [5, 5] + [6] * 28
DIST_LENS = [4, 4] + [5] * 28
WINDOW = 32768


def gzip_member(deflate, payload, flags=0, extra=b"", name=b"", comment=b""):
    """a gzip member around raw deflate bytes; flags: FHCRC 2, FEXTRA 4, FNAME 8, FCOMMENT 16"""
    h = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + b"\x00\x00\x00\x00\x00\xff")
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\x00"
    if flags & 16:
        h += comment + b"\x00"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xFFFF)
    return bytes(h) + deflate + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload) & 0xFFFFFFFF)


def raw_deflate(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_every=0, flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if not flush_every:
        return c.compress(payload) + c.flush()
    out = b""
    for o in range(0, len(payload), flush_every):
        out += c.compress(payload[o:o + flush_every]) + c.flush(flush)
    return out + c.flush()


def gz(payload, **kw):
    return gzip_member(raw_deflate(payload, **kw), payload)


class Design:
    """a deflate stream written block by block"""

    def __init__(self, seed=1):
        self.w = IC.BitWriter()
        self.out = bytearray()
        self.starts = []  # the bits at which non-final dynamic blocks begin
        self.rng = random.Random(seed)

    def bit(self):
        return len(self.w.out) * 8 + self.w.n

    def dyn(self, tokens, last=False):
        if not last:
            self.starts.append(self.bit())
        IC.dynamic_block(self.w, LIT_LENS, DIST_LENS, tokens, last=last)
        self.out = bytearray(IC.apply_tokens(tokens, bytes(self.out)))
        return self

    def stored(self, data, last=False):
        IC.stored_block(self.w, data, last=last)
        self.out += data
        return self

    def pad_to(self, byte):
        """empty stored blocks until the next block begins at or just behind `byte`"""
        while self.bit() < byte * 8:
            IC.stored_block(self.w, b"", last=False)
        return self

    def lits(self, n, alphabet=b"ACGT"):
        return [self.rng.choice(alphabet) for _ in range(n)]

    def file(self, **kw):
        return gzip_member(self.w.done(), bytes(self.out), **kw)


def model_found(starts, chunk, n_deflate):
    """{chunk index: bit} of the first designed start inside every chunk behind the first"""
    found = {}
    for s in starts:
        c = s // (8 * chunk)
        if c >= 1 and c not in found and s // 8 < n_deflate:
            found[c] = s
    return found


# ---- case 1: FASTQ text, about 1.3 MB compressed

@functools.lru_cache(maxsize=None)
def fastq_text(n_reads=17000, seed=11):
    rr = random.Random(seed)
    out = []
    for i in range(n_reads):
        n = rr.randrange(80, 121)
        out.append("@r%d/1\n%s\n+\n%s\n" % (i, "".join(rr.choices("ACGT", k=n)), "".join(rr.choices("FFFFF:,#", k=n))))
    return "".join(out).encode()


@functools.lru_cache(maxsize=None)
def fastq_gz(level):
    return gz(fastq_text(), level=level)


# ---- case 2: history across chunks, at chunks of 4 KiB.  Every named block is the first start of its chunk: the block
# in front of it begins in an earlier chunk and, where it is short, empty stored blocks carry the stream to the next chunk.
CH = 4096


@functools.lru_cache(maxsize=None)
def history_design():
    """returns (file, payload, starts, notes); notes: {name: index into starts} of the blocks the test speaks of"""
    d = Design(2)
    notes = {}

    def next_chunk():
        d.pad_to((d.bit() // (8 * CH) + 1) * CH)

    d.dyn(d.lits(40000))                                   # 45 000 bytes: chunks 0 .. 10, history full behind it
    notes["dist-32768"] = len(d.starts)
    d.dyn([(258, 32768)] + d.lits(4000))                   # the chunk's first output byte begins the match
    notes["dist-32767"] = len(d.starts)
    d.dyn([(258, 32767)] + d.lits(4000))
    notes["dist-1"] = len(d.starts)
    d.dyn([(258, 1)] + d.lits(4000))
    # a match whose source begins in front of the chunk and ends inside it, and one that ends the chunk's last block
    notes["crossing"] = len(d.starts)
    d.dyn(d.lits(100) + [(258, 200)] + d.lits(3900) + [(258, 3000)])
    notes["behind-crossing"] = len(d.starts)
    d.dyn([(258, 258), (200, 516)] + d.lits(4000))
    notes["exactly-32768"] = len(d.starts)
    d.dyn(d.lits(32768 - 258) + [(258, 20000)])
    notes["reads-all-of-it"] = len(d.starts)
    d.dyn([(258, 32768), (258, 32768 - 258 + 1)] + d.lits(32767 - 516))   # ... and produces 32 767 itself
    notes["behind-32767"] = len(d.starts)
    d.dyn([(258, 32768), (10, 32767)] + d.lits(4000))
    next_chunk()
    notes["gives-100"] = len(d.starts)
    d.pad_to((d.bit() // (8 * CH) + 1) * CH - 300)         # near its chunk's end: 100 bytes, then the next chunk
    d.dyn(d.lits(100))
    next_chunk()
    notes["behind-100"] = len(d.starts)
    d.dyn([(258, 32768), (258, 101), (258, 30000)] + d.lits(4000))   # mostly the older chunks' window
    next_chunk()
    notes["gives-nothing"] = len(d.starts)
    d.dyn([])                                              # a chunk that produces nothing
    next_chunk()
    notes["behind-nothing"] = len(d.starts)
    d.dyn([(258, 32768), (258, 1)] + d.lits(4000))
    d.dyn(d.lits(50) + [(100, 32768)], last=True)
    return d.file(), bytes(d.out), tuple(d.starts), notes


# ---- case 3: markers of markers, at chunks of 16 KiB: a line at the head, copied forward every 20 000 bytes, each copy
# from the one before
@functools.lru_cache(maxsize=None)
def relay_design():
    d = Design(3)
    line = list(b"@relay/1 the line that is handed on from chunk to chunk\n")
    d.dyn(line + d.lits(20000 - len(line)))
    for _ in range(8):
        d.dyn([(len(line), 20000)] + d.lits(20000 - len(line)))
    d.dyn([(len(line), 20000)], last=True)
    return d.file(), bytes(d.out), tuple(d.starts)


# ---- case 4: several members
@functools.lru_cache(maxsize=None)
def member_cases():
    """[(name, file, payload, members)] at chunks of 4 KiB"""
    fq = fastq_text()[:120000]
    small = dict(level=6, mem_level=4)  # (blocks of about a thousand symbols: every chunk has a start)
    a, b, c = fq[:50000], fq[50000:90000], fq[90000:]
    ma, mb, mc = gz(a, **small), gz(b, **small), gz(c, **small)
    out = [("two", ma + mb, a + b, 2), ("three", ma + mb + mc, a + b + c, 3)]
    # the second member's header on a chunk's first byte (chunks are counted from the member's first deflate byte): the
    # first member's stream is flushed, carried on by empty stored blocks and ended by an empty final one
    c1 = zlib.compressobj(6, zlib.DEFLATED, -15, 4)
    da = c1.compress(a) + c1.flush(zlib.Z_FULL_FLUSH)
    k = next(k for k in range(CH) if (len(da) + 5 * k + 5 + 8) % CH == 0)
    da += b"\x00\x00\x00\xff\xff" * k + b"\x01\x00\x00\xff\xff"
    first = gzip_member(da, a)
    assert (len(first) - 10) % CH == 0
    out.append(("on-a-chunk-boundary", first + mb, a + b, 2))
    out.append(("empty-member-between", ma + gz(b"") + mb, a + b, 3))
    out.append(("empty-member-last", ma + gz(b""), a, 2))
    out.append(("only-an-empty-member", gz(b""), b"", 1))
    hdr = gzip_member(raw_deflate(b, **small), b, flags=2 | 4 | 8 | 16, extra=b"XY\x03\x00abc", name=b"reads.fq", comment=b"a comment")
    out.append(("header-fields", ma + hdr + gzip_member(raw_deflate(c, **small), c, flags=8, name=b"c.fq"), a + b + c, 3))
    return out


# ---- case 5: files without a usable start, and flushed ones
@functools.lru_cache(maxsize=None)
def startless_cases():
    fq = fastq_text()[:200000]
    d = Design(5)
    d.dyn(d.lits(60000), last=True)
    return [("level-0", gz(fq, level=0), fq), ("fixed", gz(fq, strategy=zlib.Z_FIXED), fq),
            ("one-dynamic-block", d.file(), bytes(d.out))]


@functools.lru_cache(maxsize=None)
def flushed_cases():
    fq = fastq_text()[:300000]
    return [("sync-flush", gz(fq, flush_every=10000, flush=zlib.Z_SYNC_FLUSH), fq),
            ("full-flush", gz(fq, flush_every=10000, flush=zlib.Z_FULL_FLUSH), fq)]


# ---- case 6: a false start.  A stored block whose payload is the image of a non-final dynamic block, so placed that the
# finder of chunk 1 meets it before the true start behind it.  The payload is FASTA all the same: the image stands in a
# header line.
@functools.lru_cache(maxsize=None)
def false_start_design():
    for seed in range(50):
        img = Design(60 + seed)
        img.dyn(img.lits(40))
        image = img.w.done()
        if not any(c in image for c in b"\n\r"):
            break
    else:
        raise AssertionError("no image without a line end")
    d = Design(6)
    d.dyn(list(b">one\n") + d.lits(3000) + list(b"\n>two "))
    d.pad_to(CH + 8)
    false_bit = (len(d.w.out) + (1 if d.w.n else 0) + 4) * 8  # (the stored block's payload: behind its aligned LEN / NLEN)
    d.stored(image)
    d.dyn(list(b"\n") + d.lits(6000) + list(b"\n"))
    d.dyn(list(b">three\n") + d.lits(3000) + list(b"\n"), last=True)
    assert false_bit // (8 * CH) == 1 and d.starts[1] > false_bit
    return d.file(), bytes(d.out), false_bit


# ---- case 7: a full slot: a megabyte of one line
@functools.lru_cache(maxsize=None)
def repeated_line():
    rr = random.Random(7)
    rec = ("@same/1\n%s\n+\n%s\n" % ("".join(rr.choices("ACGT", k=100)), "I" * 100)).encode()
    payload = rec * (1000000 // len(rec))
    return gz(payload), payload


# ---- case 8: damage
def damaged(data, how):
    if how == "truncated":
        return data[:-20]
    b = bytearray(data)
    if how == "flipped-deflate-byte":
        b[len(b) // 3] ^= 0x55
    elif how == "flipped-crc-byte":
        b[-6] ^= 0x01
    else:
        raise ValueError(how)
    return bytes(b)


def small_blocks_gz(payload):
    """a .fq.gz whose blocks are about a thousand symbols (memLevel 4), so that chunks of 4 KiB find their starts"""
    return gz(payload, level=6, mem_level=4)


def self_check():
    for file, payload in ((history_design()[0], history_design()[1]), relay_design()[:2], false_start_design()[:2]):
        assert zlib.decompress(file, 31) == payload
    for _, file, payload in startless_cases() + flushed_cases():
        assert zlib.decompress(file, 31) == payload
    for _, file, payload, members in member_cases():
        assert gzip.GzipFile(fileobj=io.BytesIO(file)).read() == payload
    file, payload = repeated_line()
    assert zlib.decompress(file, 31) == payload
