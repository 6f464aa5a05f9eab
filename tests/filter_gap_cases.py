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
