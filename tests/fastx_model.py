"""A line-by-line restatement of parse_fastx (gap2seq_amd/csrc/fastx.cpp) and the read files the loader tests use.

The model follows the C++ statement by statement — LineReader.next, then the loop of parse_fastx with its two variables
`cur` and `fastq_line` — and knows nothing of the kernels' state table (csrc/fastx_machine.h).  records(data) are the
sequences of one file, text(data) the graph build's text: every sequence followed by one N."""
import gzip
import io
import random

import bamwriter


def _lines(data):
    """LineReader: a line ends at \\n or at the end of the text; one trailing \\r is dropped"""
    pos = 0
    while pos < len(data):
        e = data.find(b"\n", pos)
        if e < 0:
            e = len(data)
        line = data[pos:e]
        if len(line) > 0 and line[-1:] == b"\r":
            line = line[:-1]
        pos = e + 1
        yield line


def records(data):
    out = []
    cur = None  # index of the open record
    fastq_line = -1  # >= 0 while inside a 4-line FASTQ record
    for line in _lines(data):
        if fastq_line >= 0:
            if fastq_line == 0:
                out[cur] = line
            fastq_line += 1
            if fastq_line == 3:
                fastq_line = -1
                cur = None
            continue
        if len(line) == 0:
            continue
        if line[:1] == b">":
            out.append(b"")
            cur = len(out) - 1
        elif line[:1] == b"@" and cur is None:
            out.append(b"")
            cur = len(out) - 1
            fastq_line = 0
        elif cur is not None:
            out[cur] += line
    return out


def text(data):
    return b"".join(r + b"N" for r in records(data))


def gz(data, members=1):
    """`data` as a gzip file of `members` members, as gzip(1) writes them"""
    out = io.BytesIO()
    cut = [len(data) * i // members for i in range(members + 1)]
    for i in range(members):
        with gzip.GzipFile(fileobj=out, mode="wb", mtime=0) as f:
            f.write(data[cut[i]:cut[i + 1]])
    return out.getvalue()


def base_reads(k=31):
    """the read set of _reads(31) in tests/test_gpu_build_passes.py: about 200 reads of 400 bases with N's and lower case"""
    rr = random.Random(k)
    genome = "".join(rr.choice("ACGT") for _ in range(30000))
    reads = []
    for i in range(0, len(genome) - 400, 150):
        r = genome[i:i + 400]
        if i % 900 == 0:
            r = r[:200] + "N" + r[201:]
        if i % 1350 == 0:
            r = r.lower()
        reads.append(r)
    reads.append(genome[:k - 1])
    return genome, reads


def fasta(reads, width=0, eol="\n"):
    out = []
    for i, r in enumerate(reads):
        out.append(">read%d some comment" % i + eol)
        if width:
            out += [r[p:p + width] + eol for p in range(0, len(r), width)]
        else:
            out.append(r + eol)
    return "".join(out).encode()


def fastq(reads, eol="\n"):
    rr = random.Random(5)
    out = []
    for i, r in enumerate(reads):
        # (quality lines that begin with '@' and '>' among them: they are data, not headers)
        q = "".join(rr.choice("@>!I5+") for _ in r)
        out.append("@read%d/1%s%s%s+%s%s%s" % (i, eol, r, eol, eol, q, eol))
    return "".join(out).encode()


def base_cases():
    _, reads = base_reads()
    return [("fasta-1line", fasta(reads)), ("fasta-wrap60", fasta(reads, 60)), ("fastq", fastq(reads)),
            ("fastq-crlf", fastq(reads, "\r\n"))]


def machine_cases():
    """files of a few lines, one for every corner of the parser"""
    return [
        ("empty", b""),
        ("no-trailing-newline", b">a\nACGT\n>b\nGGCC"),
        ("trailing-cr-no-lf", b">a\nACGT\r"),
        ("lone-cr-at-end", b">a\nACGT\n\r"),
        ("cr-cr-lf", b">a\nACGT\r\r\nTT\r\n>b\r\nGG\r\r\n"),
        ("cr-inside-line", b">a\nAC\rGT\n\rACG\n"),
        ("junk-before-first", b"junk\n\nmore junk\r\n>a\nACGT\n"),
        ("junk-only", b"junk\nACGT\n\n"),
        ("header-only-records", b">a\n>b\n>c\nAC\n>d\n"),
        ("header-only-at-end-no-newline", b">a\nAC\n>"),
        ("blank-lines-in-fasta", b">a\nAC\n\n\r\nGT\n\n>b\n\nTT\n"),
        ("at-line-in-fasta", b">a\nAC\n@notaheader\nGT\n@x\nA\n+\nI\n"),
        ("fastq-qual-starts-at", b"@r1\nACGT\n+\n@III\n@r2\nGGCC\n+\n>III\n@r3\nTT\n+\nII\n"),
        ("fastq-empty-sequence", b"@r1\n\n+\n\n@r2\nAC\n+\nII\n"),
        ("fastq-empty-sequence-crlf", b"@r1\r\n\r\n+\r\n\r\n@r2\r\nAC\r\n+\r\nII\r\n"),
        ("fastq-cut-after-header", b"@r1\nAC\n+\nII\n@r2\n"),
        ("fastq-cut-after-header-no-newline", b"@r1\nAC\n+\nII\n@r2"),
        ("fastq-cut-after-sequence", b"@r1\nAC\n+\nII\n@r2\nGG"),
        ("fastq-cut-after-plus", b"@r1\nAC\n+\nII\n@r2\nGG\n+\n"),
        ("fastq-header-like-sequence", b"@r1\n>ACGT\n+\nIIIII\n@r2\n@CGT\n+\nIIII\n"),
        ("fasta-then-fastq", b">a\nACGT\n@r1\nGG\n+\nII\n>b\nTT\n"),
        ("fastq-then-fasta", b"@r1\nGG\n+\nII\n>b\nTT\nAA\n@r2\nCC\n+\nII\n"),
        ("blank-between-fastq", b"@r1\nGG\n+\nII\n\n\n@r2\nCC\n+\nII\nstray\n>c\nAA\n"),
        ("only-newlines", b"\n\n\r\n\n"),
        ("single-header-byte", b">"),
        ("single-at-byte", b"@"),
    ]


def long_line_case():
    """one line of 70 000 bases: over many pieces and over every wave and workgroup tile boundary"""
    rr = random.Random(70)
    return ("one-line-70000", b">chr\n" + bytes(rr.choice(b"ACGTN") for _ in range(70000)) + b"\n>next\nAC\n")


def many_heads_case():
    """70 000 one-base records: more line heads than bytes of anything else"""
    rr = random.Random(71)
    return ("one-base-records-70000", b"".join(b">\n" + bytes([rr.choice(b"ACGT")]) + b"\n" for _ in range(70000)))


def two_file_case():
    """a first file that ends inside a record, then a second file: the parser starts afresh"""
    return (b"@r1\nACGT\n+\nIIII\n@r2\nGGCC\n", b"+\nIIII\n>b\nTTAA\n@r3\nAC\n+\nII\n")


def compressed_cases():
    """(name, file bytes, the plain bytes they hold)"""
    plain = dict(base_cases())
    fq, crlf = plain["fastq"], plain["fastq-crlf"]
    out = [("gzip", gz(fq), fq), ("gzip-3-members", gz(fq, 3), fq), ("gzip-empty", gz(b""), b"")]
    for block in (100, 65280):
        for eof in (True, False):
            out.append(("bgzf-%d-%s" % (block, "eof" if eof else "noeof"), bamwriter.bgzf(crlf, block=block, eof=eof), crlf))
    half = len(fq) // 2
    out.append(("bgzf-then-gzip", bamwriter.bgzf(fq[:half], block=1000, eof=False) + gz(fq[half:]), fq))
    out.append(("bgzf-extra-subfield", bamwriter.bgzf(fq, block=5000, extra_first=True), fq))
    return out


def piece_sizes(data):
    """piece sizes for `data`: small ones, one that ends right behind a \\n, one that ends on the \\r of a \\r\\n, one that
    ends on a header's first byte, one larger than the file"""
    sizes = [16, 100, 1000, len(data) + 4096]
    # (the loader holds the last byte of every piece back, so the kernels' pieces end one byte before the reads do: both)
    nl = data.find(b"\n", 40)
    if nl >= 16:
        sizes += [nl + 1, nl + 2]
    cr = data.find(b"\r\n", 40)
    if cr >= 16:
        sizes += [cr + 1, cr + 2]
    for mark in (b"\n>", b"\n@"):
        h = data.find(mark, 40)
        if h >= 16:
            sizes += [h + 2, h + 3]
    return sorted(set(sizes))


def one_piece_case():
    """a FASTQ file of about 5 MiB for ONE piece: 1 300 tiles of 4 KiB, so that the two one-workgroup scans give every
    thread several tiles (no other case has more than 69)"""
    rr = random.Random(72)
    reads = ["".join(rr.choice("ACGTN") for _ in range(rr.randrange(1, 2400))) for _ in range(2200)]
    return ("fastq-5MiB", fastq(reads, "\r\n"))


def bgzf_boundary_cases():
    """(name, BGZF bytes, plain bytes, piece): members of `piece` inflated bytes, so that with that piece size every
    window is one member and the first window ends on — or right in front of — a \\r of a \\r\\n, a \\n, a header's @"""
    crlf = dict(base_cases())["fastq-crlf"]
    out = []
    cr = crlf.find(b"\r\n@", 3000)  # (\r at cr, \n at cr + 1, the next header's @ at cr + 2)
    assert cr > 0
    for name, block in (("before-cr", cr), ("on-cr", cr + 1), ("on-lf", cr + 2), ("on-header-at", cr + 3), ("behind-header-at", cr + 4)):
        out.append(("bgzf-window-ends-" + name, bamwriter.bgzf(crlf, block=block, eof=name != "on-cr"), crlf, block))
    return out
