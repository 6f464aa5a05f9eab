"""tests/bam_walk_cases.py — BAM files designed for pass A of the batched read filter (gap2seq_amd/csrc/bam_rows.hip: the
record walk and the rows on the device), and a pure-Python pass A to pin them.

Records are built here byte by byte (bamwriter.record writes no aux fields, and the cases need names without their NUL,
aux arrays that spell record heads, exact sizes); the container is bamwriter's.  A case is
    Case(name, data, windows, chunk, anomaly, raw)
`data` the BAM file, `windows` the walk windows (bytes; 0 = the reader's own) g2s_test_bam_rows is run at, `chunk` a value
for G2S_BAM_CHUNK or None, `anomaly` the RowsAnomaly the kernels must report (0: none), `raw` the inflated stream.
A walk window w cuts the first window of inflated members at first_record + w, first_record + 2 w, ...: `cut_file`
places a record's start a chosen number of bytes in front of such a cut."""
import collections
import functools
import random
import struct

import bamwriter as BW

Case = collections.namedtuple("Case", "name data windows chunk anomaly raw")

REFS = [("scaf0", 100000), ("scaf1", 50000), ("scaf2", 7000)]
MASK = (1 << 64) - 1


def header(refs=REFS):
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    raw = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for name, ln in refs:
        raw += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return raw


FIRST = len(header())


def rec(name=b"read\0", flag=0, tid=0, pos=0, cigar=(), l_seq=0, aux=b"", qual=None, mtid=-1, mpos=-1, block_size=None,
        l_name=None, seq=None):
    """one record; cigar = [(length, op)], op an index of "MIDNSHP=X"; seq bytes default to 0x88, qualities to 0xff
    (neither can be mistaken for a record head)"""
    seq = bytes([0x88]) * ((l_seq + 1) // 2) if seq is None else seq
    qual = b"\xff" * l_seq if qual is None else qual
    body = (struct.pack("<iiBBHHHiiii", tid, pos, len(name) if l_name is None else l_name, 30, 0, len(cigar), flag, l_seq,
                        mtid, mpos, 0) + name + b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar) + seq + qual + aux)
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def sized(size, **kw):
    """a record of exactly `size` bytes (block_size included), padded with aux bytes"""
    r = rec(**kw)
    assert len(r) <= size, (len(r), size)
    return rec(aux=b"\xff" * (size - len(r)), **kw)


def fake_head(block_size):
    """37 bytes that pass for the head of a record with a one-byte name: what an aux array or a quality string may spell"""
    return struct.pack("<iiiBBHHHiiii", block_size, 1, 77, 1, 0, 0, 0, 0, 0, -1, -1, 0) + b"\0"


def aux_bytes(payload):
    return b"xbBC" + struct.pack("<I", len(payload)) + payload


def container(raw, block=65280):
    return BW.bgzf(raw, block=block)


def make(name, records, windows=(0,), block=65280, chunk=None, anomaly=0, data=None, tail=b""):
    raw = header() + b"".join(records) + tail
    return Case(name, container(raw, block) if data is None else data(raw), tuple(windows), chunk, anomaly, raw)


# ---- pure-Python pass A

def std_hash(data):
    """libstdc++'s std::hash<std::string> on a 64-bit target (_Hash_bytes, seed 0xc70f6907)"""
    mul, n = 0xc6a4a7935bd1e995, len(data)
    h = (0xc70f6907 ^ (n * mul)) & MASK
    al = n & ~7
    for o in range(0, al, 8):
        d = (int.from_bytes(data[o:o + 8], "little") * mul) & MASK
        d = ((d ^ (d >> 47)) * mul) & MASK
        h = ((h ^ d) * mul) & MASK
    if n & 7:
        h = ((h ^ int.from_bytes(data[al:], "little")) * mul) & MASK
    h = ((h ^ (h >> 47)) * mul) & MASK
    return h ^ (h >> 47)


def parse(raw):
    """the rows of `raw` (an inflated BAM stream with this module's header) as the host walk makes them"""
    rows = dict(ref_id=[], pos=[], end=[], flag=[], h_own=[], h_mate=[], total=0, read_length=0, max_span=1)
    o = FIRST
    while o < len(raw):
        bs, = struct.unpack_from("<I", raw, o)
        tid, pos, l_name, _, _, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", raw, o + 4)
        assert 32 <= bs and o + 4 + bs <= len(raw)
        name = raw[o + 36:o + 36 + l_name].split(b"\0")[0]
        rlen = 0
        if not flag & 4:
            for i in range(n_cigar):
                w, = struct.unpack_from("<I", raw, o + 36 + l_name + 4 * i)
                if w & 15 in (0, 2, 3, 7, 8):
                    rlen += w >> 4
        end = pos + (rlen or 1)
        own = b"/1" if flag & 64 else b"/2"
        rows["ref_id"].append(tid)
        rows["pos"].append(pos)
        rows["end"].append(end)
        rows["flag"].append(flag)
        rows["h_own"].append(std_hash(name + own))
        rows["h_mate"].append(std_hash(name + (b"/2" if flag & 64 else b"/1")))
        rows["read_length"] = max(rows["read_length"], l_seq)
        if tid >= 0:
            rows["max_span"] = max(rows["max_span"], end - pos)
        rows["total"] += 1
        o += 4 + bs
    return rows


# ---- the name hash's probe set

def hash_names():
    """the names of the hash test, which are also the probe a process runs before its first device rows
    (name_hash_probe in readfilter_gaps.cpp builds the same list from the same generator, one draw a byte)"""
    x = [0x9E3779B97F4A7C15]

    def nxt():  # xorshift64
        v = x[0]
        v ^= (v << 13) & 0xFFFFFFFFFFFFFFFF
        v ^= v >> 7
        v ^= (v << 17) & 0xFFFFFFFFFFFFFFFF
        x[0] = v
        return v

    def printable(n):
        return bytes(33 + nxt() % 94 for _ in range(n))
    names = [printable(n) for n in range(41)]
    names.append(printable(254))
    for n in (7, 8, 9, 15, 16, 23):  # bytes >= 0x80 in each of the last seven positions (with "/1" behind: the tail's bytes)
        for back in range(1, 8):
            b = bytearray(b"a" * n)
            b[n - back] = 0x80 + nxt() % 128
            names.append(bytes(b))
    names += [b"ab\0cd", b"\0zzz", b"abcdefg\0hij\0", b"abcdefgh\0"]  # (only the part in front of the NUL counts)
    for _ in range(500):
        n = nxt() % 64
        names.append(bytes(1 + nxt() % 255 for _ in range(n)))
    return names


# ---- the designed files

def _plain(i, size=None, **kw):
    kw.setdefault("name", b"p%04d\0" % i)
    kw.setdefault("flag", 64 if i % 2 == 0 else 128)
    kw.setdefault("pos", 10 * i)
    kw.setdefault("cigar", [(20, 0)])
    kw.setdefault("l_seq", 20)
    return sized(size, **kw) if size else rec(**kw)


def cut_file(name, into, window=512, second=None, after=3):
    """a record that starts `into` bytes in front of the first cut of walk window `window`"""
    first = sized(window - into, name=b"lead\0", flag=64, pos=5, cigar=[(30, 0)], l_seq=30)
    cut = second if second is not None else _plain(1, name=b"the_cut_record\0", l_seq=40, cigar=[(40, 0)])
    return make(name, [first, cut] + [_plain(i) for i in range(2, 2 + after)], windows=(0, window))


def cut_cases():
    out = [cut_file("cut_%d_bytes_into_block_size" % x, x) for x in (1, 2, 3)]
    out.append(cut_file("cut_at_35_bytes", 35))
    out.append(cut_file("cut_at_36_bytes", 36))
    out.append(cut_file("cut_inside_the_name", 36 + 5))
    out.append(cut_file("window_ends_at_a_record_end", 0))
    out.append(cut_file("record_spans_three_windows", 100, window=256,
                        second=sized(700, name=b"long\0", flag=128, pos=9, cigar=[(200, 0)], l_seq=200)))
    recs = [_plain(i, l_seq=60, cigar=[(60, 0)]) for i in range(12)]
    out.append(make("cut_by_member_boundaries", recs, windows=(0, 300), block=250))
    # empty members (ISIZE 0) between records and inside one
    hd = header()

    def with_empty_members(raw):
        a, b = len(hd) + len(recs[0]) * 3, len(hd) + len(recs[0]) * 5 + 17
        return (BW.bgzf_block(raw[:a]) + BW.bgzf_block(b"") + BW.bgzf_block(b"") + BW.bgzf_block(raw[a:b]) + BW.bgzf_block(b"") +
                BW.bgzf_block(raw[b:]) + BW.BGZF_EOF)
    out.append(make("empty_members", recs, windows=(0, 200), data=with_empty_members))
    out.append(make("empty_members_one_a_window", recs, windows=(0,), chunk=1, data=with_empty_members))
    return out


def count_cases():
    out = []
    for n in (0, 1, 63, 64, 65):
        out.append(make("records_%d" % n, [_plain(i) for i in range(n)], windows=(0, 100)))
    out.append(make("records_4097", [_plain(i) for i in range(4097)], windows=(0, 30000), block=20000))
    return out


def field_cases():
    recs = [
        rec(name=b"no_cigar\0", flag=64, tid=1, pos=100, l_seq=10),
        rec(name=b"clips_only\0", flag=128, tid=1, pos=200, cigar=[(5, 4), (3, 1), (2, 5), (1, 6)], l_seq=8),
        rec(name=b"every_op\0", flag=64 | 16, tid=2, pos=300, cigar=[(10, 0), (2, 2), (300, 3), (4, 7), (5, 8), (6, 1), (7, 4)], l_seq=32),
        rec(name=b"unmapped_with_cigar\0", flag=64 | 4, tid=0, pos=50, cigar=[(90, 0)], l_seq=90),
        rec(name=b"no_bases\0", flag=128, tid=0, pos=60, cigar=[(12, 0)], l_seq=0),
        rec(name=b"\0", flag=64, tid=0, pos=70, cigar=[(9, 0)], l_seq=9),
        rec(name=b"n" * 254 + b"\0", flag=128, tid=0, pos=80, cigar=[(9, 0)], l_seq=9),
        rec(name=b"inner\0nul_x\0", flag=64, tid=0, pos=90, cigar=[(9, 0)], l_seq=9),
        rec(name=b"inner\0", flag=128, tid=0, pos=91, cigar=[(9, 0)], l_seq=9),
        rec(name=b"neither_end\0", flag=0, tid=0, pos=95, cigar=[(9, 0)], l_seq=9),
        rec(name=b"high\xe9\xff\x80\0", flag=64, tid=0, pos=96, cigar=[(9, 0)], l_seq=9),
        rec(name=b"odd_bases\0", flag=128, tid=2, pos=6000, cigar=[(33, 0)], l_seq=33),
        rec(name=b"aux\0", flag=64, tid=2, pos=6100, cigar=[(8, 0)], l_seq=8, aux=b"NMC\x03XZhello\0"),
        rec(name=b"nowhere\0", flag=128 | 4 | 8, tid=-1, pos=-1, l_seq=25),
    ]
    out = [make("fields", recs, windows=(0, 150))]
    big = dict(cigar=[(500, 0)], l_seq=120)
    small = [_plain(i) for i in range(1, 6)]
    out.append(make("maxima_by_the_first_record", [_plain(0, **big)] + small, windows=(0, 150)))
    out.append(make("maxima_by_the_last_record", small + [_plain(9, **big)], windows=(0, 150)))
    out.append(make("maxima_by_a_record_without_reference",
                    small + [rec(name=b"far\0", flag=64, tid=-1, pos=1000, cigar=[(900, 0)], l_seq=300)], windows=(0, 150)))
    return out


def false_start_cases():
    """aux arrays and quality strings that spell whole record heads: (a) linked to a true record's start, (b) to another
    false head, (c) to nowhere, (d) past the window"""
    def carrier(i, payload):
        return rec(name=b"carrier%d\0" % i, flag=64, tid=0, pos=1000 + i, cigar=[(15, 0)], l_seq=15, aux=aux_bytes(payload))
    lead = _plain(0)
    pre = len(carrier(0, b""))  # bytes of a carrier in front of its payload
    gap = 60
    # (a): the head's record would end exactly where the carrier ends, i.e. on the next true record
    a = carrier(1, b"\xee" * 7 + fake_head(gap + 37 - 4 + 0) + b"\xee" * gap)
    # (b): two heads in one array, the first linked to the second; the second to nowhere (c)
    b = carrier(2, b"\xee" * 3 + fake_head(33 + 20) + b"\xee" * 20 + fake_head(33 + 50) + b"\xee" * 90)
    # (d): far past everything
    d = carrier(3, fake_head(1 << 20) + b"\xee" * 30)
    q = rec(name=b"qual_head\0", flag=128, tid=1, pos=40, cigar=[(80, 0)], l_seq=80, qual=fake_head(36 + 80 - 37 - 4 + 33)[:37] + b"\x21" * 43)
    recs = [lead, a, _plain(1), b, _plain(2), d, _plain(3), q, _plain(4)]
    assert a[pre + 7:pre + 11] == struct.pack("<i", gap + 33)
    # a walk window that starts two bytes in front of (a)'s false head: the head lies right behind the window's first bytes
    at = len(lead) + pre + 7 - 2
    out = [make("false_starts", recs, windows=(0, at, 256, 100))]
    # many false heads in a row (an array of them): more than one candidate a true record, none of them a row
    many = carrier(4, b"".join(fake_head(33 + 11) + b"\xee" * 11 for _ in range(40)))
    out.append(make("false_starts_in_a_row", [lead, many] + [_plain(i) for i in range(5, 9)], windows=(0, 333)))
    return out


def _dense_heads(n):
    """n bytes in which every 16th offset starts a plausible head: block_size 65536 (and n_cigar 0), reference 0,
    position 0, a one-byte name"""
    unit = struct.pack("<iiii", 65536, 0, 0, 1)
    return (unit * (n // 16 + 1))[:n]


def anomaly_cases():
    out = []
    big = rec(name=b"long_read\0", flag=64, tid=0, pos=100, cigar=[(300000, 0)], l_seq=300000)
    out.append(make("carry_longer_than_the_front", [_plain(0), big, _plain(1), _plain(2)], windows=(0,), chunk=100000, anomaly=3))
    out.append(make("name_without_its_nul", [_plain(0), rec(name=b"abcd", flag=64, tid=0, pos=7, cigar=[(9, 0)], l_seq=9), _plain(1)],
                    windows=(0, 100), anomaly=1))
    dense = rec(name=b"dense\0", flag=128, tid=0, pos=9, cigar=[(10, 0)], l_seq=8000, qual=_dense_heads(8000))
    out.append(make("more_candidates_than_the_capacity", [_plain(0), dense, _plain(1)], windows=(4096,), block=4096, chunk=4096,
                    anomaly=2))
    return out


@functools.lru_cache(maxsize=None)
def designed_cases():
    return tuple(cut_cases() + count_cases() + field_cases() + false_start_cases())


@functools.lru_cache(maxsize=None)
def handed_over_cases():
    return tuple(anomaly_cases())


def error_cases():
    """(name, data, chunk, message): files the host walk rejects; the public calls must say the same with device rows"""
    good = [_plain(i, l_seq=50, cigar=[(50, 0)]) for i in range(6)]
    last = _plain(7, l_seq=50, cigar=[(50, 0)])
    out = [("truncated_in_the_body", container(header() + b"".join(good) + last[:-20]), None, "truncated BAM record"),
           ("truncated_in_block_size", container(header() + b"".join(good) + last[:2]), None, "truncated BAM record"),
           ("block_size_31", container(header() + b"".join(good) + struct.pack("<i", 31) + b"\0" * 31), None, "bad BAM record size"),
           ("l_name_0", container(header() + b"".join(good) + rec(name=b"", l_seq=4) + good[0]), None, "bad BAM record layout"),
           ("layout_beyond_block_size", container(header() + b"".join(good) + rec(name=b"x\0", l_seq=4, block_size=36) + good[0]), None,
            "bad BAM record layout")]
    import inflate_cases as IC
    many = [_plain(i, l_seq=200, cigar=[(200, 0)], seq=bytes(random.Random(i).randrange(256) for _ in range(100))) for i in range(200)]
    data = container(header() + b"".join(many), block=5000)
    members = IC.split_members(data)
    m = bytearray(members[6])
    m[-5] ^= 0x10  # (a bit of its CRC-32)
    out.append(("corrupt_member_in_the_second_window", b"".join(members[:6]) + bytes(m) + b"".join(members[7:]), 20000,
                "corrupt BGZF block 6"))
    return out
