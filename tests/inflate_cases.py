"""tests/inflate_cases.py — BGZF members designed for the inflaters of gap2seq_amd/csrc (inflate_core.h on the host,
g2s_bgzf_inflate on the device, zlib): what zlib.compressobj can be asked for comes from it; what it will not emit on
request is written bit by bit (RFC 1951).  valid_cases() / corrupt_cases() return (name, member bytes[, payload]);
self_check() inflates every valid design with Python's zlib and makes sure that it rejects every corrupt one, so that a
wrong design fails where it is written and not on the GPU.

A member is at most 65 536 bytes in the file (its size minus one is a 16-bit field), so 65 536 stored bytes do not fit
one: the 65 536-byte member with two stored blocks carries 60 000 bytes in them and matches for the rest, and the largest
level-0 member here has 65 280 bytes."""
import functools
import random
import struct
import zlib

import bamwriter as BW

EOF = BW.BGZF_EOF


def member(deflate, payload, crc=None, isize=None):
    crc = zlib.crc32(payload) & 0xFFFFFFFF if crc is None else crc
    isize = len(payload) if isize is None else isize
    bsize = len(deflate) + 26
    assert bsize <= 65536, bsize
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + deflate +
            struct.pack("<II", crc, isize))


def split_members(data):
    out, o = [], 0
    while o < len(data):
        n = struct.unpack_from("<H", data, o + 16)[0] + 1
        out.append(data[o:o + n])
        o += n
    return out


def zlib_inflate(m):
    """the payload of one member as Python's zlib sees it; raises ValueError when it is no valid member"""
    xlen, = struct.unpack_from("<H", m, 10)
    crc, isize = struct.unpack_from("<II", m, len(m) - 8)
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(m[12 + xlen:len(m) - 8], isize + 1)
    except zlib.error as e:
        raise ValueError(str(e))
    if not d.eof or len(out) != isize:
        raise ValueError("size")
    if zlib.crc32(out) & 0xFFFFFFFF != crc:
        raise ValueError("crc")
    return out


def deflate(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if flush_at is None:
        return c.compress(payload) + c.flush()
    return c.compress(payload[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[flush_at:]) + c.flush()


# ---- bits

class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, k):  # a field, least significant bit first
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):  # a Huffman code, most significant bit first
        for i in range(k - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def len_sym(n):
    s = 28 if n == 258 else max(i for i in range(28) if LEN_BASE[i] <= n)
    return s, n - LEN_BASE[s]


def dist_sym(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, d - DIST_BASE[s]


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (no completeness check: corrupt designs too)"""
    code, out = 0, {}
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                out[s] = (code, ln)
                code += 1
        code <<= 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def apply_tokens(tokens, out=b""):
    out = bytearray(out)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert 1 <= d <= len(out)
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def put_tokens(w, tokens, lit, dist):
    """tokens: a byte value, or (length, distance); then the end-of-block code"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        else:
            n, d = t
            s, x = len_sym(n)
            w.code(*lit[257 + s])
            w.bits(x, LEN_EXTRA[s])
            s, x = dist_sym(d)
            w.code(*dist[s])
            w.bits(x, DIST_EXTRA[s])
    w.code(*lit[256])


def fixed_block(w, tokens, last=True):
    w.bits(1 if last else 0, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(w, data, last=True, nlen=None):
    w.bits(1 if last else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack("<HH", len(data), (~len(data) & 0xFFFF) if nlen is None else nlen) + data)


# the code-length code every dynamic block here uses: symbols 0..12 in 4 bits, 13..18 in 5 (complete)
CL_LENS = [4] * 13 + [5] * 6
CL_CODE = canonical(CL_LENS)


def rle_lengths(seq):
    """the combined literal/length + distance lengths as code-length symbols, greedy with 16 / 17 / 18 over the WHOLE
    list (so repeats run across the boundary between the two codes wherever the values allow it)"""
    out, i = [], 0
    while i < len(seq):
        v = seq[i]
        run = 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            n = min(run, 138)
            out.append((18, n - 11, 7, i, n) if n >= 11 else (17, n - 3, 3, i, n))
            i += n
        elif i > 0 and seq[i - 1] == v and run >= 3:
            n = min(run, 6)
            out.append((16, n - 3, 2, i, n))
            i += n
        else:
            out.append((v, 0, 0, i, 1))
            i += 1
    return out


def dynamic_block(w, lit_lens, dist_lens, tokens, last=True, crossing=None):
    """crossing: the code-length symbol (16, 17 or 18) that must run across the boundary between the two codes"""
    assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
    w.bits(1 if last else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257, 5)
    w.bits(len(dist_lens) - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(CL_LENS[s], 3)
    rle = rle_lengths(list(lit_lens) + list(dist_lens))
    if crossing is not None:
        assert any(s == crossing and at < len(lit_lens) < at + n for s, _, _, at, n in rle), rle
    for s, x, xb, _, _ in rle:
        w.code(*CL_CODE[s])
        w.bits(x, xb)
    put_tokens(w, tokens, canonical(lit_lens), canonical(dist_lens))


def lens_of(assign, n):
    v = [0] * n
    for s, l in assign.items():
        v[s] = l
    return v


def _rand(n, seed):
    return random.Random(seed).randbytes(n)


def _text(n, seed):
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"acgtnACGT") for _ in range(rng.randrange(2, 9))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
    return bytes(out[:n])


def _designed():
    """(name, deflate bytes, payload)"""
    A, B, C = 97, 98, 99
    out = []
    # literals only, one distance code of zero length
    w = BitWriter()
    toks = [A, B, A, C, A, A, B]
    dynamic_block(w, lens_of({A: 1, B: 2, C: 3, 256: 3}, 257), [0], toks)
    out.append(("dynamic_literals_only", w.done(), apply_tokens(toks)))
    # a single distance code (one symbol, one bit: the incomplete code zlib accepts)
    w = BitWriter()
    toks = [A, (10, 1), B, (3, 1)]
    dynamic_block(w, lens_of({A: 2, B: 2, 256: 2, 257: 3, 264: 3}, 265), [1], toks)
    out.append(("single_distance_code", w.done(), apply_tokens(toks)))
    # codes of 15 bits, literal/length and distance
    w = BitWriter()
    ll = {256: 15, 65: 15}
    for i, s in enumerate([A, B, C, 100, 101, 102, 103, 104, 105, 106, 107, 257, 258, 285]):
        ll[s] = i + 1
    dl = list(range(1, 15)) + [15, 15]
    toks = [A, B, C, 100, 101, 102, 103, 104, 105, 106, 107, 65] * 30 + [(3, 1), (4, DIST_BASE[14]), (258, DIST_BASE[15] + 3), 65]
    dynamic_block(w, lens_of(ll, 286), dl, toks)
    out.append(("codes_of_15_bits", w.done(), apply_tokens(toks)))
    # 16 / 17 / 18 running from the literal/length lengths into the distance lengths
    for sym, lit, dist in ((16, lens_of({A: 2, B: 2, 256: 2, 257: 2}, 258), [2, 2, 2, 2]),
                           (17, lens_of({A: 2, B: 2, 256: 2, 257: 2}, 260), [0, 0, 2, 2, 2, 2]),
                           (18, lens_of({A: 1, B: 2, 256: 3, 257: 3}, 270), [0] * 6 + [2, 2, 2, 2])):
        w = BitWriter()
        first = next(i for i, l in enumerate(dist) if l)
        toks = [A, B, B, A, A, B, A, A] * 4 + [(3, DIST_BASE[first]), (3, DIST_BASE[first + 3]), B]
        dynamic_block(w, lit, dist, toks, crossing=sym)
        out.append(("repeat_%d_crosses_the_codes" % sym, w.done(), apply_tokens(toks)))
    # length 258 at short distances, and around one wave of lanes
    for d in (1, 2, 3, 63, 64, 65):
        w = BitWriter()
        toks = list(_rand(d + 5, 100 + d)) + [(258, d), 33, (258, d), (258, 1)]
        fixed_block(w, toks)
        out.append(("match_258_at_distance_%d" % d, w.done(), apply_tokens(toks)))
    # distance 32 768 exactly, from the member's first byte
    w = BitWriter()
    head = _rand(32768, 7)
    stored_block(w, head, last=False)
    toks = [(258, 32768), 1, (100, 32768), (3, 32768)]
    fixed_block(w, toks)
    out.append(("distance_32768_from_the_first_byte", w.done(), apply_tokens(toks, head)))
    # matches whose source or destination lies across a multiple of 64 output bytes
    w = BitWriter()
    toks = list(_rand(60, 8))
    for at in (62, 63, 64, 65, 126, 127, 128, 129, 190, 256, 320):
        cur = len(apply_tokens(toks))
        toks += list(_rand((at - cur) % 64, at))  # the matches below begin `at` bytes behind a multiple of 64
        cur = len(apply_tokens(toks))
        toks += [(7, 3), (70, cur - 30), (5, 66), (130, 5), (64, 64), (65, 63), (3, cur)]
    fixed_block(w, toks)
    out.append(("matches_across_multiples_of_64", w.done(), apply_tokens(toks)))
    # length 3 at the last three bytes of a 65 536-byte member (two stored blocks in front)
    w = BitWriter()
    head = _rand(60000, 9)
    stored_block(w, head[:30000], last=False)
    stored_block(w, head[30000:], last=False)
    toks = [(258, 1000)] * 21 + [(115, 32768)] + [(3, 32768)]
    body = apply_tokens(toks, head)
    assert len(body) == 65536, len(body)
    fixed_block(w, toks)
    out.append(("length_3_at_the_end_of_65536", w.done(), body))
    # several blocks of every kind in one member, an empty stored block between them
    w = BitWriter()
    fixed_block(w, [A, B, (5, 2)], last=False)
    stored_block(w, b"", last=False)
    dynamic_block(w, lens_of({A: 1, B: 2, C: 3, 256: 3}, 257), [0], [C, A, B], last=False)
    stored_block(w, b"xyz", last=False)
    fixed_block(w, [(6, 3)], last=True)
    out.append(("blocks_of_every_kind", w.done(), apply_tokens([A, B, (5, 2), C, A, B, 120, 121, 122, (6, 3)])))
    return out


@functools.lru_cache(maxsize=None)
def valid_cases():
    """(name, member, payload)"""
    out = [(n, member(d, p), p) for n, d, p in _designed()]
    for size in (0, 1, 63, 64, 65, 65280, 65535, 65536):
        p = _text(size, size)
        out.append(("default_%d" % size, member(deflate(p), p), p))
    for size in (1, 64, 5000, 65280):
        p = _rand(size, size + 1)
        out.append(("stored_%d" % size, member(deflate(p, level=0), p), p))
    p = _text(5000, 3)
    out.append(("stored_in_small_blocks", member(deflate(p, level=0, mem_level=1), p), p))
    for size in (1, 65, 40000):
        p = _text(size, size + 2)
        out.append(("fixed_%d" % size, member(deflate(p, strategy=zlib.Z_FIXED), p), p))
    p = _text(30000, 4) + _rand(2000, 5) + b"\0" * 9000
    out.append(("full_flush_in_the_middle", member(deflate(p, flush_at=17000), p), p))
    p = b"A" * 65536
    out.append(("one_byte_run_65536", member(deflate(p, level=9), p), p))
    return out


def valid_file(eof=True):
    cases = valid_cases()
    return b"".join(m for _, m, _ in cases) + (EOF if eof else b""), b"".join(p for _, _, p in cases)


@functools.lru_cache(maxsize=None)
def corrupt_cases():
    """(name, member): each is rejected by zlib, or fails its trailer"""
    A, B = 97, 98
    out = []
    p = _text(3000, 11)
    d = deflate(p)
    out.append(("truncated_deflate", member(d[:len(d) // 2], p)))
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    for t in (1, 2, 3, 4, 5):
        w.code(*FIXED_LIT[t])
    w.code(*FIXED_LIT[257])  # length 3 ...
    w.code(*FIXED_DIST[4])   # ... at distance 6 (symbol 4: 5 + one extra bit), one beyond the five bytes there are
    w.bits(1, 1)
    w.code(*FIXED_LIT[256])
    out.append(("distance_beyond_the_output", member(w.done(), bytes([1, 2, 3, 4, 5, 1, 2, 3]))))
    for name, assign in (("oversubscribed_literal_lengths", {A: 1, B: 1, 256: 1}),
                         ("incomplete_length_code", {A: 2, B: 2, 256: 2}),
                         ("no_end_of_block_code", {A: 1, B: 1})):
        w = BitWriter()
        lit = lens_of(assign, 257)
        w.bits(1, 1)
        w.bits(2, 2)
        w.bits(0, 5)
        w.bits(0, 5)
        w.bits(15, 4)
        for s in CL_ORDER:
            w.bits(CL_LENS[s], 3)
        for s, x, xb, _, _ in rle_lengths(lit + [0]):
            w.code(*CL_CODE[s])
            w.bits(x, xb)
        code = canonical(lit)
        for t in (A, B, A):
            w.code(*code[t])
        if 256 in code:
            w.code(*code[256])
        w.bits(0, 16)
        out.append((name, member(w.done(), bytes([A, B, A]))))
    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 29)
    out.append(("block_type_3", member(w.done(), b"abc")))
    w = BitWriter()
    stored_block(w, b"abcdef", nlen=(~6 & 0xFFFF) ^ 0x0100)
    out.append(("len_nlen_mismatch", member(w.done(), b"abcdef")))
    p = _text(2000, 12)
    out.append(("one_more_byte_than_isize", member(deflate(p), p[:-1], isize=len(p) - 1)))
    out.append(("one_fewer_byte_than_isize", member(deflate(p), p + b"x", isize=len(p) + 1)))
    out.append(("flipped_crc_bit", member(deflate(p), p, crc=(zlib.crc32(p) & 0xFFFFFFFF) ^ 0x00100000)))
    return out


def corrupt_file(bad):
    """three members, the bad one in the middle"""
    p, q = _text(700, 21), _rand(300, 22)
    return member(deflate(p), p) + bad + member(deflate(q, level=0), q) + EOF


def good_file_after():
    p, q = _text(900, 23), _text(65280, 24)
    return member(deflate(p), p) + member(deflate(q), q) + EOF, p + q


def self_check():
    for name, m, p in valid_cases():
        assert zlib_inflate(m) == p, name
    for name, m in corrupt_cases():
        try:
            zlib_inflate(m)
        except ValueError:
            continue
        raise AssertionError("Python's zlib accepts the corrupt design " + name)


@functools.lru_cache(maxsize=None)
def random_corpus(seed=20240611, n=200):
    """(file, payload): about n members of text, runs, random bytes and BAM records at levels 0 / 1 / 6 / 9 and Z_FIXED"""
    rng = random.Random(seed)
    refs, recs, _ = BW.simulate_library(seed, n_scaffolds=1, scaffold_len=4000, pairs=400, unmapped_pairs=10)
    bam = b"".join(recs)
    members, payload = [], []
    for i in range(n):
        kind = i % 4
        size = rng.choice([rng.randrange(1, 300), rng.randrange(300, 9000), rng.randrange(9000, 65281)])
        if kind == 0:
            p = _text(size, seed + i)
        elif kind == 1:
            p = b"".join(bytes([rng.randrange(256)]) * rng.randrange(1, 600) for _ in range(size // 200 + 1))[:size]
        elif kind == 2:
            p = _rand(min(size, 20000), seed + i)
        else:
            o = rng.randrange(0, max(1, len(bam) - size))
            p = bam[o:o + size]
        how = rng.randrange(5)
        d = deflate(p, strategy=zlib.Z_FIXED) if how == 4 else deflate(p, level=[0, 1, 6, 9][how])
        if len(d) + 26 > 65536:
            d = deflate(p)
        members.append(member(d, p))
        payload.append(p)
    return b"".join(members) + EOF, b"".join(payload)
