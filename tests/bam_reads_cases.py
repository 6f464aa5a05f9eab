"""tests/bam_reads_cases.py — BAM files as read files of the graph build (gap2seq_amd/csrc/bam_reads.h): the cases and a
model of the definition.  The model decodes the records bamwriter wrote, byte by byte, never through the product: every
record that is neither secondary (0x100) nor supplementary (0x800) gives its bases — codes 1, 2, 4, 8 are A, C, G, T,
every other code N, a reverse-strand record (0x10) reverse-complemented — followed by 'N'."""
import random
import struct

import bamwriter

REFS = [("scaffold_one", 100000), ("scaffold_two", 50000), ("scaffold_three", 7)]
FWD = "NACNGNNNTNNNNNNN"
REV = "NTGNCNNNANNNNNNN"
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)


def read_of(rec):
    """the sequence one written record contributes, or None for a record that is skipped"""
    bs, = struct.unpack_from("<i", rec, 0)
    assert bs + 4 == len(rec)
    l_name = rec[12]
    n_cigar, flag, l_seq = struct.unpack_from("<HHi", rec, 16)
    if flag & 0x900:
        return None
    packed = rec[36 + l_name + 4 * n_cigar:]
    codes = [(packed[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)]
    if flag & 16:
        return "".join(REV[c] for c in reversed(codes))
    return "".join(FWD[c] for c in codes)


def reads(records):
    return [r for r in map(read_of, records) if r is not None]


def text(records):
    return "".join(r + "N" for r in reads(records)).encode()


def first_record(refs=REFS, header_text="@HD\tVN:1.6\tSO:coordinate\n"):
    """the inflated offset of the first alignment record of bamwriter.bam_bytes(refs, ...)"""
    t = header_text + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    return 12 + len(t) + sum(8 + len(name) + 1 for name, _ in refs)


def _seq(rr, n, alphabet="ACGT"):
    return "".join(rr.choice(alphabet) for _ in range(n))


def _rec(rr, i, seq, flag=0, name=None):
    name = name if name is not None else "r%d" % i + "x" * (i % 3)  # (names of even and odd length)
    if flag & 4:
        return bamwriter.record(name, flag, -1, -1, "", seq)
    return bamwriter.record(name, flag, i % 2, 10 + i, "%dM" % len(seq) if seq else "", seq)


def length_records(seed=1):
    """every length forward and reverse, under names of even and odd length"""
    rr = random.Random(seed)
    out = []
    for n in LENGTHS:
        for flag in (0, 16, 4, 16 | 1 | 64):
            for name in ("ab", "abc"):
                out.append(_rec(rr, len(out), _seq(rr, n, "ACGTN"), flag, name + str(len(out) % 10)))
    return out


def code_records():
    """all sixteen codes, forward and reverse, at even and odd length"""
    all16 = bamwriter.SEQ_CODES
    return [bamwriter.record(name, flag, 0, 5, "%dM" % len(s), s)
            for name in ("c", "cc") for flag in (0, 16) for s in (all16, all16[::-1] + "A", all16 * 9)]


def skipped_records(seed=2):
    """secondary and supplementary records first, last, in a run of more than 64, and alternating with kept ones"""
    rr = random.Random(seed)
    out = [_rec(rr, 0, _seq(rr, 40), 0x100), _rec(rr, 1, _seq(rr, 41), 0x800 | 16)]
    for i in range(10):
        out.append(_rec(rr, len(out), _seq(rr, 30 + i), 16 if i % 3 == 0 else 0))
    for i in range(70):
        out.append(_rec(rr, len(out), _seq(rr, 20 + i % 7), 0x100 if i % 2 else 0x800))
    for i in range(40):
        out.append(_rec(rr, len(out), _seq(rr, 35), (0, 0x100, 16, 0x900 | 16)[i % 4]))
    out.append(_rec(rr, len(out), _seq(rr, 50), 0x800))
    return out


def only_skipped_records(seed=3):
    rr = random.Random(seed)
    return [_rec(rr, i, _seq(rr, 30), 0x100 if i % 2 else 0x800) for i in range(5)]


def row_records(n, seed=4):
    """n kept rows of short reads, a skipped record now and then"""
    rr = random.Random(seed + n)
    out = []
    for i in range(n):
        out.append(_rec(rr, i, _seq(rr, 1 + i % 9), 16 if i % 5 == 0 else 0, "q%d" % (i % 100)))
        if i % 50 == 7:
            out.append(_rec(rr, i, _seq(rr, 5), 0x100, "s"))
    return out


def library_records(seed=6):
    refs, recs, _ = bamwriter.simulate_library(seed, n_scaffolds=1, scaffold_len=2000, gap=(900, 150), pairs=60, unmapped_pairs=5,
                                               ambiguous=0.2)
    return refs, recs


def cases():
    """[(name, BAM bytes, records, window sizes for the device route)]: a window holds the header at the least"""
    first = first_record()
    hold = (first + 99) // 100 * 100  # the smallest window of 100-byte members that holds the header
    assert first > 100  # (the header spans members)
    std = (1000, 20000, 0)
    small = (hold, 1000, 1 << 20)
    out = [
        ("no-record", [], {}, std),
        ("only-skipped", only_skipped_records(), {}, std),
        ("lengths", length_records(), {}, std),
        ("codes", code_records(), {}, std),
        ("skipped", skipped_records(), {}, std),
        ("rows-63", row_records(63), {}, std),
        ("rows-64", row_records(64), {}, std),
        ("rows-65", row_records(65), {}, std),
        ("rows-4097", row_records(4097), {}, (20000, 0)),
        ("lengths-members-100", length_records(), dict(block=100), small),
        ("skipped-members-100", skipped_records(), dict(block=100), small),
        ("lengths-members-100-no-eof", length_records(7), dict(block=100, eof=False), small),
        ("no-record-members-100", [], dict(block=100), small),
    ]
    out = [(name, bamwriter.bam_bytes(REFS, recs, **args), recs, pieces) for name, recs, args, pieces in out]
    refs, recs = library_records()
    out.append(("library", bamwriter.bam_bytes(refs, recs, block=3000), recs, (4000, 0)))
    return out


def graph_reads(k, seed=11):
    """(genome, records): reads of a random genome as an aligner would leave them — forward and reverse records, unmapped
    ones, ambiguity codes, secondary and supplementary copies in between — enough of them for solid k-mers at solid 2"""
    rr = random.Random(seed * 1000 + k)
    genome = _seq(rr, 12000)
    recs = []
    for i, at in enumerate(range(0, len(genome) - 300, 100)):
        s = genome[at:at + 300 + i % 2]
        if i % 7 == 0:
            s = s[:150] + "R" + s[151:]
        flag = (0, 16, 4, 1 | 64 | 16)[i % 4]
        stored = bamwriter.revcomp(s.replace("R", "N")) if flag & 16 else s
        recs.append(_rec(rr, i, stored, flag))
        if i % 9 == 0:  # (a copy the aligner wrote a second time: it must not count twice)
            recs.append(_rec(rr, i, stored[:120], flag | (0x100 if i % 2 else 0x800)))
    recs.append(_rec(rr, len(recs), "", 4))
    recs.append(_rec(rr, len(recs), genome[:k - 1], 0))
    return genome, recs
