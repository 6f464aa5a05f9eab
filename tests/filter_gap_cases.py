"""Cases of the batched read filter (g2s_filter_reads_gaps) shared by tests/test_readfilter_gaps.py (host joins) and
tests/test_gpu_readfilter_gaps.py (device joins): every case is one library — (bam bytes, mean, std_dev, gaps) — and
every gap's output must equal the per-gap filter's (g2s_filter_reads) and the restatement's
(oracle/readfilter_ref.py)."""
import base64
import json
import os
import random

import bamwriter as BW
import readfilter_ref as REF

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    """tests/golden/readfilter_cases.json: every call of one library setting as one batch"""
    g = json.load(open(os.path.join(HERE, "golden", "readfilter_cases.json")))
    bam = base64.b64decode(g["bam_base64"])
    groups = {}
    for c in g["calls"]:
        a = c["args"]
        if a.get("unmapped_only"):
            continue
        groups.setdefault((a["mean"], a["std_dev"]), []).append(
            (a["scaffold"], a["breakpoint"], a.get("gap_length", -1), a.get("flank_length", -1)))
    return [(bam, mean, sd, gaps) for (mean, sd), gaps in sorted(groups.items())]


def mixed_gaps(rng, scaffolds, count):
    """breakpoints all over the scaffolds (windows clipped at 0 included), flank -1 / 0 / > 0, gap length -1 / 0 / > 0,
    an unknown scaffold, and two gaps at the same breakpoint"""
    gaps = []
    for i in range(count):
        scaf = rng.choice(scaffolds)
        bp = rng.choice([rng.randrange(0, 3000), rng.randrange(0, 200), 1400])
        gl = rng.choice([-1, 0, rng.randrange(1, 300)])
        fl = rng.choice([-1, 0, rng.randrange(1, 150)])
        gaps.append((scaf, bp, gl, fl))
    gaps.append(("nosuch", 1400, 200, 100))
    gaps.append((scaffolds[0], 1400, 200, 100))
    gaps.append((scaffolds[0], 1400, 200, 100))  # (the same breakpoint twice)
    gaps.append((scaffolds[-1], 1400, 150, -1))
    gaps.append((scaffolds[0], 20, 10, 200))      # (every window clipped at 0)
    return gaps


def simulated(seed, shuffle=False, n_scaffolds=3, pairs=250, block=65280, gaps=24):
    rng = random.Random(seed)
    refs, recs, _ = BW.simulate_library(seed, n_scaffolds=n_scaffolds, pairs=pairs, ambiguous=0.05)
    if shuffle:  # a file whose records are not coordinate-sorted (its header still says SO:coordinate)
        recs = list(recs)
        rng.shuffle(recs)
    bam = BW.bam_bytes(refs, recs, block=block)
    return bam, [r[0] for r in refs], mixed_gaps(rng, [r[0] for r in refs], gaps)


def collision():
    """A library where the name of a read far from every window collides, modulo 5 x records, with the name the left
    window puts into the filter: the batched filter must extract it (the reference's one-bit Bloom filter does).
    Returns (bam, mean, sd, gaps, the colliding read's FASTA header)."""
    refs = [("s", 5000)]
    base = [BW.record("w", 1 | 64 | 8, 0, 600, "50M", "A" * 50, 0, 600),          # in the left window, mate unmapped
            BW.record("w", 1 | 128 | 4, 0, 600, "", "C" * 50, 0, 600),            # its mate
            BW.record("d", 1 | 64, 0, 3000, "50M", "G" * 50, 0, 3300),
            BW.record("d", 1 | 128 | 16, 0, 3300, "50M", "T" * 50, 0, 3000)]
    bits = 5 * (len(base) + 1)
    want = REF.std_hash(b"w/1") % bits
    for i in range(100000):
        name = "c%d" % i
        if REF.std_hash((name + "/1").encode()) % bits == want and REF.std_hash((name + "/2").encode()) % bits != want:
            break
    else:
        raise AssertionError("no colliding name found")
    recs = base + [BW.record(name, 1 | 128, 0, 4000, "50M", "ACGT" * 12 + "AC", 0, 4500)]  # its mate name is name/1
    bam = BW.bam_bytes(refs, recs)
    # window [bp - (mean + 2 rl), bp - (mean + rl)) = [600, 650) with rl = 50, mean = 300: bp = 1000
    return bam, 300, 0, [("s", 1000, 100, -1), ("s", 1000, 100, 30), ("s", 2000, 100, 30)], ">%s/2\n" % name


def empty_window_library():
    """std_dev 0 makes the right-hand window [x, x), x = bp + mean + read length + gap length; a mate-unmapped read
    spans x.  An empty region holds nothing (htslib, readfilter_ref._query)."""
    refs = [("s", 5000)]
    recs = [BW.record("a", 1 | 64 | 8, 0, 1430, "50M", "A" * 50, 0, 1430),   # spans x = 1000 + 300 + 50 + 100 = 1450
            BW.record("a", 1 | 128 | 4, 0, 1430, "", "C" * 50, 0, 1430),
            BW.record("b", 1 | 64, 0, 3000, "50M", "G" * 50, 0, 3200),
            BW.record("b", 1 | 128 | 16, 0, 3200, "50M", "T" * 50, 0, 3000)]
    return BW.bam_bytes(refs, recs), 300, 0, [("s", 1000, 100, -1), ("s", 1000, 100, 20)]


def empty_bam():
    return BW.bam_bytes([("s", 100)], []), 100, 10, [("s", 50, 5, 10), ("nosuch", 50, 5, -1)]


def _window_mates(bam, mean, sd, scaf, bp, gl):
    """the mate-unmapped records in the left and in the right window of a gap, by the restatement's own query"""
    refs, recs = REF.parse_bam(bam)
    tid = refs.index(scaf)
    rl = max(r.l_seq for r in recs)
    left = REF._query(recs, tid, bp - (mean + 3 * sd + 2 * rl), bp - (mean - 3 * sd + rl), [])
    right = REF._query(recs, tid, bp + (mean + 3 * sd + rl) + gl, bp + (mean - 3 * sd + rl) + gl, [])
    return [r for r in left if r.flag & 8], [r for r in right if r.flag & 8]


def sd_negative(sd):
    """A negative standard deviation makes the right-hand window, whose bounds the reference writes the wrong way
    round, a non-empty [beg, end): the only setting in which it holds a record.  The gaps are chosen, with the
    restatement, so that one has mate-unmapped records in its right window and one in its left window."""
    refs, recs, _ = BW.simulate_library(5, n_scaffolds=1, pairs=600)
    bam = BW.bam_bytes(refs, recs)
    gaps, seen = [], [0, 0]
    for bp in range(300, 2700, 50):
        for gl in (200, 50):
            left, right = _window_mates(bam, 300, sd, "scaf0", bp, gl)
            if (left and seen[0] < 2) or (right and seen[1] < 2):
                seen[0] += bool(left)
                seen[1] += bool(right)
                gaps += [("scaf0", bp, gl, -1), ("scaf0", bp, gl, 60)]
    assert seen[0] >= 1 and seen[1] >= 1, seen
    return bam, 300, sd, gaps + mixed_gaps(random.Random(sd), ["scaf0"], 6)


def _library(rng, tid, lo, hi, pairs, prefix, length=lambda: 50, p_mu=0.3):
    """[((tid, pos), record)] of a small paired library on one reference: both ends aligned, or one end unmapped and
    placed at its mate"""
    out = []

    def seq(n):
        return "".join(rng.choice("ACGT") for _ in range(n))
    for i in range(pairs):
        name = "%s%04d" % (prefix, i)
        a, l1, l2 = rng.randrange(lo, hi), length(), length()
        first, second = (64, 128) if rng.random() < 0.5 else (128, 64)
        if rng.random() < p_mu:
            out.append(((tid, a), BW.record(name, 1 | first | 8, tid, a, "%dM" % l1, seq(l1), tid, a)))
            out.append(((tid, a), BW.record(name, 1 | second | 4, tid, a, "", seq(l2), tid, a)))
        else:
            b = a + rng.randrange(100, 400)
            out.append(((tid, a), BW.record(name, 1 | first | 32, tid, a, "%dM" % l1, seq(l1), tid, b)))
            out.append(((tid, b), BW.record(name, 1 | second | 16, tid, b, "%dM" % l2, seq(l2), tid, a)))
    return out


def _sorted_bam(refs, keyed, **args):
    order = sorted(range(len(keyed)), key=lambda i: (keyed[i][0], i))
    return BW.bam_bytes(refs, [keyed[i][1] for i in order], **args)


def long_span():
    """Records with N and D operations spanning 2 000 to 20 000 reference bases that begin far to the left of the
    windows they reach, among ordinary reads: the longest span is 400 times the read length."""
    rng = random.Random(41)
    keyed = _library(rng, 0, 0, 59000, 500, "r")
    long_ones = [("L0", 10000, "20M5000N30M", 8), ("L1", 20000, "10M19990D40M", 8), ("L2", 30000, "25M2000N25M", 0),
                 ("L3", 30500, "5S20M12000N10M3D15M", 8), ("L4", 100, "30M9000N20M", 0)]
    for name, pos, cigar, mu in long_ones:
        keyed.append(((0, pos), BW.record(name, 1 | 64 | mu, 0, pos, cigar, "ACGTA" * 10, 0, pos)))
        if mu:
            keyed.append(((0, pos), BW.record(name, 1 | 128 | 4, 0, pos, "", "TTGCA" * 10, 0, pos)))
    bam = _sorted_bam([("s", 60000)], keyed)
    # left window [bp - 400, bp - 350), right window (sd 0) empty, flanks [bp - fl, bp + fl + gl)
    gaps = [("s", 15400, 100, 40), ("s", 40380, 100, 40), ("s", 42900, 50, 100), ("s", 32020, 10, 30), ("s", 9100, 20, 60),
            ("s", 15450, 100, 40), ("s", 25000, 100, -1), ("s", 12000, 100, 500)]
    for bp, name in ((15400, "L0"), (40380, "L1"), (42900, "L3")):  # the long record's unmapped mate is extracted
        left, _ = _window_mates(bam, 300, 0, "s", bp, 100)
        assert any(r.name == name.encode() for r in left), (bp, name)
        assert ">%s/2\n" % name in REF.read_filter(bam, 300, 0, "s", bp, 100, 40)[0]
    assert ">L2/1\n" in REF.read_filter(bam, 300, 0, "s", 32020, 10, 30)[0]     # in the flanks, 2 000 bases from its start
    assert ">L4/1\n" in REF.read_filter(bam, 300, 0, "s", 9100, 20, 60)[0]
    assert ">L0/2\n" not in REF.read_filter(bam, 300, 0, "s", 15450, 100, 40)[0]  # [15050, 15100): at L0's end, not in it
    return bam, 300, 0, gaps


def mixed_lengths():
    """reads of 30 to 150 bases: the windows follow the longest l_seq (150), which is not the longest span (a 150-base
    read with a deletion of 300)"""
    rng = random.Random(43)
    keyed = _library(rng, 0, 0, 5500, 500, "m", length=lambda: rng.randrange(30, 151))
    keyed += _library(rng, 1, 0, 2500, 200, "n", length=lambda: rng.randrange(30, 151))
    keyed.append(((0, 2000), BW.record("del", 1 | 64 | 8, 0, 2000, "100M300D50M", "ACGTAC" * 25, 0, 2000)))
    keyed.append(((0, 2000), BW.record("del", 1 | 128 | 4, 0, 2000, "", "T" * 30, 0, 2000)))
    keyed.append(((0, 10), BW.record("longest", 1 | 64, 0, 10, "150M", "G" * 150, 0, 300)))
    bam = _sorted_bam([("a", 6000), ("b", 3000)], keyed, block=900)
    refs, recs = REF.parse_bam(bam)
    assert max(r.l_seq for r in recs) == 150 and min(r.l_seq for r in recs) <= 35
    assert max(r.end_pos() - r.pos for r in recs) == 450
    # left window [bp - 660, bp - 390) at sd 20; bp = 3100: [2440, 2710) holds `del` by its last 10 bases only
    left, _ = _window_mates(bam, 300, 20, "a", 3100, 100)
    assert any(r.name == b"del" for r in left)
    return bam, 300, 20, [("a", 3100, 100, 80), ("a", 3100, 100, -1)] + mixed_gaps(rng, ["a", "b"], 20)


def repeated_names():
    """Secondary (256) and supplementary (2048) copies of a mate-unmapped read inside the left window, and a pair of
    which neither record carries READ1: both are called name/2 and both look for name/1."""
    rng = random.Random(47)
    keyed = _library(rng, 0, 0, 4500, 300, "r")
    for pos, extra in ((620, 0), (625, 256), (640, 2048), (3000, 256)):
        keyed.append(((0, pos), BW.record("dup", 1 | 64 | 8 | extra, 0, pos, "50M", "ACGTT" * 10, 0, 620)))
    keyed.append(((0, 620), BW.record("dup", 1 | 128 | 4, 0, 620, "", "GGCCA" * 10, 0, 620)))
    keyed.append(((0, 630), BW.record("noend", 1 | 8, 0, 630, "50M", "A" * 50, 0, 630)))      # neither READ1 ...
    keyed.append(((0, 630), BW.record("noend", 1 | 4, 0, 630, "", "C" * 50, 0, 630)))          # ... nor its mate
    keyed.append(((0, 1010), BW.record("both1", 1 | 64, 0, 1010, "50M", "G" * 50, 0, 1200)))   # both READ1
    keyed.append(((0, 1200), BW.record("both1", 1 | 64 | 16, 0, 1200, "50M", "T" * 50, 0, 1010)))
    bam = _sorted_bam([("s", 5000)], keyed)
    left, _ = _window_mates(bam, 300, 0, "s", 1000, 100)   # [600, 650)
    assert sum(1 for r in left if r.name == b"dup") == 3 and any(r.name == b"noend" for r in left)
    fa = REF.read_filter(bam, 300, 0, "s", 1000, 100, 30)[0]
    assert fa.count(">dup/2\n") == 1 and ">noend/2\n" not in fa.split(">dup/2\n")[0]
    return bam, 300, 0, [("s", 1000, 100, -1), ("s", 1000, 100, 30), ("s", 3400, 100, 30)] + mixed_gaps(rng, ["s"], 8)


def placed_at_minus_one():
    """records with a reference and position -1 (end position 0 without a CIGAR, 49 with 50M), and gaps whose windows
    are clipped at 0"""
    rng = random.Random(53)
    keyed = _library(rng, 0, 0, 2500, 200, "r")
    keyed.append(((0, -1), BW.record("neg", 1 | 64 | 8, 0, -1, "50M", "ACGTG" * 10, 0, -1)))
    keyed.append(((0, -1), BW.record("neg", 1 | 128 | 4, 0, -1, "", "TTACA" * 10, 0, -1)))
    keyed.append(((0, -1), BW.record("neg2", 1 | 64 | 4 | 8, 0, -1, "", "CCACA" * 10, 0, -1)))
    bam = _sorted_bam([("s", 3000)], keyed)
    left, _ = _window_mates(bam, 300, 0, "s", 380, 100)    # [-20, 30) -> [0, 30)
    assert [r.name for r in left if r.pos == -1] == [b"neg"]  # (end 49 > 0; the two that end at 0 are not in [0, 30))
    return bam, 300, 0, [("s", 380, 100, -1), ("s", 380, 100, 400), ("s", 350, 0, 0), ("s", 20, 10, 200), ("s", 0, 0, 1),
                         ("s", 400, 100, 10)]


def many_scaffolds():
    rng = random.Random(59)
    refs = [("c%04d" % i, 3000) for i in range(3000)]
    keyed = []
    for tid in (0, 1, 1499, 1500, 2998, 2999):
        keyed += _library(rng, tid, 0, 2500, 60, "t%d_" % tid, p_mu=0.4)
    bam = _sorted_bam(refs, keyed)
    gaps = []
    for name in ("c0000", "c1500", "c2999", "c0002", "c1499"):
        gaps += [(name, 1400, 200, 100), (name, 900, 100, -1), (name, 2100, 50, 300)]
    for name in ("c0000", "c1500", "c2999"):
        assert any(_window_mates(bam, 300, 20, name, bp, gl)[0] for _, bp, gl, _ in gaps[:3]), name
    return bam, 300, 20, gaps


def high_coordinates():
    """a reference of 2^31 - 1 bases with reads and gaps at its end: positions, window ends and flanks at and beyond
    INT32_MAX"""
    top = (1 << 31) - 1
    rng = random.Random(61)
    keyed = _library(rng, 0, top - 3000, top - 450, 300, "h", p_mu=0.4)
    keyed += _library(rng, 0, 0, 3000, 50, "l")
    keyed.append(((0, top - 1), BW.record("last", 1 | 64 | 8, 0, top - 1, "1M", "A", 0, top - 1)))
    keyed.append(((0, top - 1), BW.record("last", 1 | 128 | 4, 0, top - 1, "", "ACGTC" * 10, 0, top - 1)))
    bam = _sorted_bam([("big", top)], keyed)
    gaps = [("big", top - 1200, 100, 100), ("big", top - 300, 200, 400), ("big", top, 1000, 2000), ("big", top - 2000, 50, -1),
            ("big", top - 1, top, top), ("big", 1400, 100, 100)]
    assert _window_mates(bam, 300, 20, "big", top - 1200, 100)[0]
    assert _window_mates(bam, 300, -8, "big", top - 2000, 100)[1]     # (and a populated right-hand window up there)
    return bam, 300, 20, gaps


def all_cases():
    """(label, bam, mean, sd, gaps)"""
    out = [("golden-%d-%d" % (m, s), b, m, s, g) for b, m, s, g in golden()]
    for seed, shuffle, block in ((1, False, 65280), (2, True, 700), (3, True, 97)):
        bam, _, gaps = simulated(seed, shuffle=shuffle, block=block)
        out.append(("sim%d" % seed, bam, 300, 20, gaps))
    bam, _, gaps = simulated(4, shuffle=True)
    out.append(("sim4-sd0", bam, 300, 0, gaps))
    bam, mean, sd, gaps, _ = collision()
    out.append(("collision", bam, mean, sd, gaps))
    out.append(("empty-window",) + empty_window_library())
    out.append(("empty-bam",) + empty_bam())
    bam, _, _ = simulated(5)
    out.append(("n1", bam, 250, 40, [("scaf1", 1400, 200, 100)]))
    out.append(("sd-negative-5",) + sd_negative(-5))
    out.append(("sd-negative-8",) + sd_negative(-8))
    out.append(("long-span",) + long_span())
    out.append(("mixed-lengths",) + mixed_lengths())
    out.append(("repeated-names",) + repeated_names())
    out.append(("placed-at-minus-one",) + placed_at_minus_one())
    out.append(("many-scaffolds",) + many_scaffolds())
    bam, mean, sd, gaps = high_coordinates()
    out.append(("high-coordinates", bam, mean, sd, gaps))
    out.append(("high-coordinates-sd-negative", bam, mean, -8, [("big", (1 << 31) - 2001, 100, 100), ("big", (1 << 31) - 1500, 10, -1)]))
    return out


def expected(P, bam, mean, sd, gaps, restatement=True):
    """every gap's (fasta, log, warn, extracted, total) from the per-gap filter, checked against the restatement"""
    want = []
    for scaf, bp, gl, fl in gaps:
        got = P.filter_reads(bam, mean=mean, std_dev=sd, scaffold=scaf, breakpoint=bp, gap_length=gl, flank_length=fl)
        if restatement:
            assert got[:3] == REF.read_filter(bam, mean, sd, scaf, bp, gl, fl), (scaf, bp, gl, fl)
        want.append(got)
    return want
