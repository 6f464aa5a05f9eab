"""tests/bam_store_cases.py — the store route of the batched read filter's one-pass mode (gap2seq_amd/csrc/bam_store.h): a
pure-Python compaction written from the format, the plan of the two capacities restated, and two files designed to
overflow one planned capacity each.

A stored record is the source's 36 head bytes with block_size rewritten to 32 + l_name + ceil(l_seq / 2) and n_cigar_op
(bytes 16-17) to 0, then the l_name name bytes, then the packed bases; records lie back to back."""
import functools
import struct

import bam_walk_cases as WC

SAMPLE = 1 << 20          # the sample's bytes behind the header (G2S_FILTER_STORE_SAMPLE changes it)
OVERFLOW_SAMPLE = 16384   # what the overflow files are designed for


def source_records(raw):
    """(offset, block_size, l_name, n_cigar, l_seq) of every record of an inflated stream with WC's header"""
    out, o = [], WC.FIRST
    while o < len(raw):
        bs, = struct.unpack_from("<I", raw, o)
        _, _, l_name, _, _, n_cigar, _, l_seq = struct.unpack_from("<iiBBHHHi", raw, o + 4)
        out.append((o, bs, l_name, n_cigar, l_seq))
        o += 4 + bs
    return out


def stored_bytes(l_name, l_seq):
    return 36 + l_name + (l_seq + 1) // 2


def compact(raw):
    """(the store, every record's offset in it) of an inflated stream"""
    store, offs = bytearray(), []
    for o, _, l_name, n_cigar, l_seq in source_records(raw):
        offs.append(len(store))
        head = bytearray(raw[o:o + 36])
        head[0:4] = struct.pack("<I", stored_bytes(l_name, l_seq) - 4)
        head[16:18] = b"\0\0"
        seq = o + 36 + l_name + 4 * n_cigar
        store += head + raw[o + 36:o + 36 + l_name] + raw[seq:seq + (l_seq + 1) // 2]
    return bytes(store), offs


def sample_of(raw, sample=SAMPLE):
    """(r, z, c): the records that begin in the first `sample` bytes behind the header, the bytes they cover (the last one
    whole), their stored bytes"""
    lim = WC.FIRST + min(sample, len(raw) - WC.FIRST)
    r = z = c = 0
    for o, bs, l_name, _, l_seq in source_records(raw):
        if o >= lim:
            break
        r, z, c = r + 1, z + 4 + bs, c + stored_bytes(l_name, l_seq)
    return r, z, c


def ceil_div(a, b):
    return -(-a // b)


def plan(P, r, z, c):
    """dict(rows_cap, store_cap, need) by the rule: a margin of 1.25 on the sample's densities, an additive term each,
    neither beyond the worst case"""
    rows = (ceil_div(5 * r * P, 4 * z) if z and r else 0) + 64
    store = (ceil_div(5 * c * P, 4 * z) if z and c else 0) + 4096
    rows_cap, store_cap = min(P // 36 + 1, rows), min(P, store)
    return dict(rows_cap=rows_cap, store_cap=store_cap, need=52 * (rows_cap + 1) + store_cap)


def plan_of(raw, sample=SAMPLE):
    r, z, c = sample_of(raw, sample)
    out = plan(len(raw) - WC.FIRST, r, z, c)
    out.update(sample_records=r, sample_bytes=z, sample_stored=c)
    return out


def _small(i, **kw):
    return WC.rec(flag=64 if i % 2 == 0 else 128, tid=0, pos=i, **kw)


@functools.lru_cache(maxsize=None)
def rows_overflow():
    """the sample: records of 290 bytes with 254-byte names and no bases, every byte of them stored, so that store_cap
    reaches P; behind it 2 000 records of 48 bytes: six times the sample's records a byte"""
    recs = [_small(i, name=b"n" * 249 + b"%04d\0" % i) for i in range(60)]
    recs += [_small(i, name=b"r%04d\0" % i, l_seq=4) for i in range(2000)]
    return WC.make("store_rows_overflow", recs)


@functools.lru_cache(maxsize=None)
def store_overflow():
    """the sample: records of 291 bytes with 5-byte names and 250 bytes of tags, 41 bytes of each stored; behind it 2 000
    records of 290 bytes with 254-byte names and no tags, every byte of them stored: the same records a byte, seven times
    the stored share"""
    recs = [_small(i, name=b"s%03d\0" % i, aux=b"\xff" * 250) for i in range(60)]
    recs += [_small(i, name=b"n" * 249 + b"%04d\0" % i) for i in range(2000)]
    return WC.make("store_store_overflow", recs)
