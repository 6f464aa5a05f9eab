"""tests/bam_text_cases.py — BAM files designed for pass B of the batched read filter (gap2seq_amd/csrc/bam_text.hip: the
bases, names and FASTA text of selected records), and a pure-Python pass B written from the format to pin them.

The records are bam_walk_cases.rec's, with their 4-bit bases given byte by byte.  The lengths are the ones at which a
wave's 64-byte steps, the odd last nibble and the reversed read order can go wrong."""
import functools
import random
import struct

import bam_walk_cases as WC
import bamwriter as BW

REVERSE, READ1, READ2, UNMAPPED = 16, 64, 128, 4
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 3001)
ALL_CODES = bytes(range(16))

FWD = "NACNGNNNTNNNNNNN"   # SAM specification 4.2.3: "=ACMGRSVTWYHKDBN"; A, C, G, T stay, the rest is N
REV = "NTGNCNNNANNNNNNN"   # ... and the complement, for a record aligned to the reverse strand


def pack(codes):
    """4-bit codes, high nibble first, the odd last one in a high nibble"""
    c = list(codes) + ([0] if len(codes) % 2 else [])
    return bytes(c[i] << 4 | c[i + 1] for i in range(0, len(c), 2))


def _rec(name, flag, codes, pos):
    return WC.rec(name=name, flag=flag, tid=0, pos=pos, cigar=[(max(1, len(codes)), 0)], l_seq=len(codes), seq=pack(codes))


@functools.lru_cache(maxsize=None)
def designed_records():
    rng = random.Random(20250101)
    recs, pos = [], 100
    for n in LENGTHS:
        for strand in (0, REVERSE):
            codes = [rng.randrange(16) for _ in range(n)]
            recs.append(_rec(b"len%d_%d\0" % (n, strand), strand | rng.choice((READ1, READ2, 0)), codes, pos))
            pos += 7
    for strand in (0, REVERSE):  # all 16 codes, at even and at odd length
        recs.append(_rec(b"codes\0", strand | READ1, ALL_CODES, pos))
        recs.append(_rec(b"codes_odd\0", strand | READ2, ALL_CODES[:15], pos + 1))
        pos += 7
    recs.append(_rec(b"x\0", READ1, [1, 2, 4, 8], pos))
    recs.append(_rec(b"y" * 254 + b"\0", READ2 | REVERSE, [1, 2, 4, 8, 15], pos + 1))
    recs.append(_rec(b"ab\0cd\0", READ1, [8, 4, 2], pos + 2))
    recs.append(_rec(b"\0tail\0", 0, [2], pos + 3))  # (a name that is empty in front of its first NUL)
    for flag in (READ1, READ2, 0, READ1 | READ2, UNMAPPED | READ1, UNMAPPED | REVERSE):
        recs.append(_rec(b"flag%d\0" % flag, flag, [rng.randrange(16) for _ in range(70)], pos + 4))
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def designed():
    """Case(name, data, windows, chunk, anomaly, raw) of bam_walk_cases, one file of every designed record"""
    return WC.make("text_designed", list(designed_records()), block=900)


@functools.lru_cache(maxsize=None)
def small_files():
    return (WC.make("text_records_0", []), WC.make("text_records_1", [designed_records()[8]]))


def recut(case, window):
    """`case` with its inflated stream cut into members, and by G2S_BAM_CHUNK into reader windows of one member each, where
    the walk window `window` cuts it in bam_walk_cases: at first_record + window, first_record + 2 * window, ..."""
    raw, cut = case.raw, WC.FIRST + window
    members = [raw[:cut]] + [raw[o:o + window] for o in range(cut, len(raw), window)]
    data = b"".join(BW.bgzf_block(m) for m in members) + BW.BGZF_EOF
    return WC.Case("%s_recut_%d" % (case.name, window), data, (0,), window, case.anomaly, raw)


@functools.lru_cache(maxsize=None)
def window_cases():
    """the designed files of bam_walk_cases as they are, and cut into reader windows at each of their walk windows"""
    out = []
    for case in WC.designed_cases():
        out.append(case)
        out += [recut(case, w) for w in case.windows if w]
    return tuple(out)


def selections(n):
    """(name, rows) for a file of n records: empty, every row, the first, the last, alternating, and a list out of order
    with repeats"""
    out = [("none", []), ("all", list(range(n)))]
    if n:
        out += [("first", [0]), ("last", [n - 1]), ("alternating", list(range(0, n, 2))), ("odd", list(range(1, n, 2)))]
    if n > 3:
        out.append(("unordered_repeats", [n - 1, 2, 2, 0, n - 1]))
    return out


def records(raw):
    """(name bytes in front of the first NUL, flag, codes) of every record of an inflated stream with WC's header"""
    out, o = [], WC.FIRST
    while o < len(raw):
        bs, = struct.unpack_from("<I", raw, o)
        _, _, l_name, _, _, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", raw, o + 4)
        name = raw[o + 36:o + 36 + l_name].split(b"\0")[0]
        seq = raw[o + 36 + l_name + 4 * n_cigar:][:(l_seq + 1) // 2]
        out.append((name, flag, [(seq[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)]))
        o += 4 + bs
    return out


def bases_of(flag, codes):
    if flag & REVERSE:
        return "".join(REV[c] for c in reversed(codes)).encode()
    return "".join(FWD[c] for c in codes).encode()


def name_of(name, flag):
    return name + (b"/1" if flag & READ1 else b"/2")


def expected(raw, rows, names=True, fasta=False):
    """what lib.bam_text returns for the records `rows` of `raw`"""
    recs = records(raw)
    B, N, bo, no = b"", b"", [0], [0]
    for r in sorted(set(rows)):
        name, flag, codes = recs[r]
        if fasta:
            B += b">" + name_of(name, flag) + b"\n" + bases_of(flag, codes) + b"\n"
        else:
            B += bases_of(flag, codes)
            if names:
                N += name_of(name, flag)
                no.append(len(N))
        bo.append(len(B))
    return dict(bases=B, base_off=bo, names=N, name_off=no if names and not fasta else None)
