"""tests/bam_stream_cases.py — the streaming form of the BAM read route (gap2seq_amd/csrc/bam_reads.h): a model of where
its windows end, which field of which record an end cuts, the documented bound of its fixed device footprint, and the
file of 250-base reads that is over the resident cap.  Nothing here goes through the product."""
import random
import struct

import bam_reads_cases as B
import bamwriter

FRONT = 256 << 10  # room in front of an inflate window (csrc/bam.cpp: kDeviceFront)
FIELDS = ("fixed", "name", "cigar", "bases", "qualities")


def hold():
    """the smallest window of 100-byte members that holds the header (bam_reads_cases.cases)"""
    return (B.first_record() + 99) // 100 * 100


def window_ends(raw_len, block, piece, first=None):
    """the inflated offsets at which walk windows end, in a stream of raw_len bytes written in members of `block` bytes
    and read with a window of `piece` bytes: an inflate window takes whole members while they fit (one at the least), and
    is walked `piece` bytes at a time — the first from the first record's offset"""
    first = B.first_record() if first is None else first
    members = [min(block, raw_len - o) for o in range(0, raw_len, block)]
    windows, at = [], 0
    while at < len(members):
        e, size = at, 0
        while e < len(members) and (e == at or size + members[e] <= piece):
            size += members[e]
            e += 1
        windows.append(size)
        at = e
    walk = min(piece, max(windows))
    ends, base = [], 0
    for w, size in enumerate(windows):
        ws = first if w == 0 else 0
        while ws < size:
            ws = min(ws + walk, size)
            ends.append(base + ws)
        base += size
    return ends


def field_at(rec, rel):
    """the field of a written record that holds its byte `rel`"""
    l_name = rec[12]
    n_cigar, _, l_seq = struct.unpack_from("<HHi", rec, 16)
    bounds = (36, 36 + l_name, 36 + l_name + 4 * n_cigar, 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2, len(rec))
    for name, b in zip(FIELDS, bounds):
        if rel < b:
            return name
    raise AssertionError("beyond the record")


def cut_fields(recs, block, piece):
    """the fields in which a window's end falls, with at least one byte of the record in front of it"""
    starts, o = [], B.first_record()
    for r in recs:
        starts.append(o)
        o += len(r)
    hit, i = set(), 0
    for e in window_ends(o, block, piece):
        while i + 1 < len(starts) and starts[i + 1] <= e:
            i += 1
        if starts and starts[i] < e < starts[i] + len(recs[i]):
            hit.add(field_at(recs[i], e - starts[i]))
    return hit


def renamed(rec, name):
    """a written record under another name: the same read from a longer record"""
    nm = name.encode() + b"\0"
    assert len(nm) <= 255
    body = rec[4:12] + bytes([len(nm)]) + rec[13:36] + nm + rec[36 + rec[12]:]
    return struct.pack("<i", len(body)) + body


def fixed_bound(piece, block):
    """csrc/bam_reads.h: 2 * (F + 2 * w' + 64 * (m + 1)) + 64 * (w / 36 + 66) + 64 KiB bounds the streaming form's fixed
    footprint for windows of w bytes; w' <= max(w, 64 KiB) the largest window of whole members, m its members"""
    members = max(piece // block, 1)
    largest = members * block
    return 2 * (FRONT + 2 * largest + 64 * (members + 1)) + 64 * (piece // 36 + 66) + (64 << 10)


def device_text_bytes(t):
    """csrc/reads_text.h: the bytes a text of t positions needs"""
    return (t + 16383) // 16384 * 16384 + 128


def big_reads(min_stream, seed=23):
    """(genome, records): 250-base reads of a random genome as bam_reads_cases.graph_reads leaves them, enough of them for
    an inflated stream of at least min_stream bytes behind the header"""
    rr = random.Random(seed)
    step, per_record = 25, 36 + 4 + 4 + 125 + 250
    genome = "".join(rr.choices("ACGT", k=step * (min_stream // per_record + 64) + 300))
    recs, size = [], 0
    for i, at in enumerate(range(0, len(genome) - 250, step)):
        s = genome[at:at + 250]
        if i % 11 == 0:
            s = s[:100] + "R" + s[101:]
        flag = (0, 16, 4, 1 | 64 | 16)[i % 4]
        stored = bamwriter.revcomp(s.replace("R", "N")) if flag & 16 else s
        name = "r%d" % i
        recs.append(bamwriter.record(name, flag, -1, -1, "", stored) if flag & 4 else
                    bamwriter.record(name, flag, i % 2, 10 + i, "250M", stored))
        size += len(recs[-1])
        if i % 97 == 0:  # (a copy the aligner wrote a second time: it must not count twice)
            recs.append(bamwriter.record(name, flag | 0x100, 0, 10 + i, "100M", stored[:100]))
            size += len(recs[-1])
        if size >= min_stream:
            break
    assert size >= min_stream
    return genome, recs
