"""tests/cases.py — seeded toy inputs shared by the CPU and GPU test suites.
Own tiny PRNG (SplitMix64) so fixtures never depend on Python's `random`."""


class SplitMix:
    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def randint(self, lo, hi):
        return lo + self.next() % (hi - lo + 1)

    def choice(self, seq):
        return seq[self.next() % len(seq)]

    def random(self):
        return (self.next() >> 11) / float(1 << 53)


def random_dna(rng, n):
    return "".join("ACGT"[rng.next() & 3] for _ in range(n))


def toy_genome(seed, length, k, repeats=0, tandem=0, inverted=0, snp_every=0):
    """Returns list of read sequences (haplotypes) forming the DBG, first one is the
    genome gaps are cut from.  repeats: dispersed exact copies; tandem: tandem
    arrays (cycles -> non-trivial SCCs); inverted: reverse-complement copies
    (Q7 territory); snp_every: second haplotype with substitutions (bubbles)."""
    rng = SplitMix(seed * 7919 + 13)
    g = list(random_dna(rng, length))
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for _ in range(repeats):
        ln = rng.randint(k + 2, 4 * k)
        src = rng.randint(0, length - ln - 1)
        dst = rng.randint(0, length - ln - 1)
        g[dst:dst + ln] = g[src:src + ln]
    for _ in range(tandem):
        unit = rng.randint(max(2, k // 2), 2 * k)
        copies = rng.randint(3, 6)
        src = rng.randint(0, length - unit * copies - 1)
        u = g[src:src + unit]
        for c in range(copies):
            g[src + c * unit:src + (c + 1) * unit] = u
    for _ in range(inverted):
        ln = rng.randint(k + 2, 3 * k)
        src = rng.randint(0, length - ln - 1)
        dst = rng.randint(0, length - ln - 1)
        g[dst:dst + ln] = [comp[c] for c in reversed(g[src:src + ln])]
    g = "".join(g)
    seqs = [g]
    if snp_every:
        h = list(g)
        p = snp_every // 2
        while p < length:
            h[p] = rng.choice([c for c in "ACGT" if c != h[p]])
            p += snp_every + rng.randint(0, 5)
        seqs.append("".join(h))
    return seqs


def one_strand_genome(seed, length, alphabet="AC"):
    """A genome over A and C only: the reverse complement of every k-mer is made of T and G, so no k-mer ever
    meets its own reverse strand and NO gap is a Q7 case — at k = 5 or 7 the toy genomes of
    toy_genome() make nearly every gap one, and Q7 gaps are outside the bit-exact comparison.  With 2^k
    possible k-mers the graph is dense: dozens of cycles per closure, path counts that saturate at MAX_PATHS."""
    rng = SplitMix(seed * 7919 + 13)
    return "".join(alphabet[rng.randint(0, len(alphabet) - 1)] for _ in range(length))


def cut_gaps(seed, genome, k, fuz, ngaps, min_len, max_len, d_err, vary_fuz=True, claim_noise=True):
    """List of dicts(left,right,gap_len,lmf,rmf,true_len).  The claimed gap length is
    chosen so that most gaps are fillable: the DP accepts path lengths
    g + lmf + j +- err with err <= d_err while the true path is true_len + k + lmf
    long (Gap2Seq.cpp:1125-1126), so claimed = true_len + k + noise."""
    rng = SplitMix(seed * 104729 + 7)
    out = []
    n = len(genome)
    for _ in range(ngaps):
        gl = rng.randint(min_len, max_len)
        lmf = rmf = fuz
        if vary_fuz and rng.random() < 0.25:
            rmf = rng.randint(0, fuz)
        if vary_fuz and rng.random() < 0.25:
            lmf = rng.randint(0, fuz)
        pos = rng.randint(k + lmf, n - gl - k - rmf - 1)
        claimed = gl
        if claim_noise:
            claimed = gl + k + rng.choice([0, 0, 0, -d_err, d_err, -(d_err // 2), d_err // 2, d_err + 1, -(d_err + 1), -k])
        claimed = max(1, claimed)
        out.append(dict(left=genome[pos - k - lmf:pos], right=genome[pos + gl:pos + gl + k + rmf], gap_len=claimed,
                        lmf=lmf, rmf=rmf, true_len=gl))
    return out


def clean_haplotypes(seqs, k):
    """True when no k-mer is its own reverse complement, no k-mer meets its reverse strand anywhere in the
    haplotypes and no haplotype holds a k-mer twice: what several haplotypes share is the same oriented k-mer."""
    comp = str.maketrans("ACGT", "TGCA")
    seen = {}
    for h, s in enumerate(seqs):
        for i in range(len(s) - k + 1):
            x = s[i:i + k]
            y = x.translate(comp)[::-1]
            if x == y:
                return False
            at = seen.setdefault(min(x, y), (x, h, i))
            if at[0] != x or (at[1] == h and at[2] != i):
                return False
    return True


def bubble_ladder(seed, k, m, spacing, indel=False, lead=0, tail=0, out_tips=(), in_tips=(), fuz=3):
    """A chain of m bubbles between two flanks, with tips added on demand.  Returns dict(seqs, gap, bubbles, paths):
    seqs[0] is the random backbone, seqs[1] a second haplotype with m substitutions `spacing` (>= k + 1) bases apart,
    the first `lead` bases after the left flank's last k-mer and the last `tail` bases in front of the right flank's
    first k-mer; gap is the cut_gaps-style record of the one gap from the backbone's first k + fuz bases to its last.

    Closure shape (k-mers, not bases): every substitution gives a bubble of two arms of k k-mers each; between two
    bubbles the haplotypes share spacing - k k-mers, one unitig.  The left DP therefore logs one segment per arm and
    one per shared stretch: about 3 segments per bubble, 2^m paths of one length (the count saturates at MAX_PATHS
    from m = 30 on).  With indel=True every third bubble is a deletion on haplotype 2 instead (arms of k and k - 1
    k-mers): later unitigs are entered at two depths, the paths have several lengths, and the closure has k-mers at
    several depths (the fill kernels leave it to phase D2 on the device or to the host).

    out_tips: backbone offsets (from the left flank's last k-mer) at which a dead end of k + 2 bases branches off
    (a third read that leaves the backbone): in the left half of the gap each cuts one unitig in two and adds the
    tip's own segment: +2 logged segments, no right-set entry.  in_tips: offsets at which a source of k + 2 bases
    joins the backbone (a read that ends on it): the backbone's unitig is cut (+1 logged segment) and the tip is
    one more predecessor for phase A to enter (+1 right-set entry when it lies in the right half).  Seeds whose
    haplotypes repeat a k-mer anywhere (either strand) are rejected and the next seed of the stream is tried."""
    assert spacing >= k + 1
    rng = SplitMix(seed * 6151 + 101)
    fl = k + fuz
    n = fl + lead + (m - 1) * spacing + 1 + tail + fl if m else fl + lead + tail + fl
    for _ in range(1000):
        g = random_dna(rng, n)
        h = list(g)
        bubbles = []
        for b in range(m):
            p = fl + lead + b * spacing
            if indel and b % 3 == 2:
                h[p] = ""
            else:
                h[p] = "ACGT"[("ACGT".index(h[p]) + 1 + rng.randint(0, 2)) % 4]
            bubbles.append(p)
        seqs = [g, "".join(h)] if m else [g]
        for t in out_tips:  # the backbone up to offset t, then a fresh k + 2 bases: a dead end behind fl + t
            p = fl + t
            seqs.append(g[p - k:p + 1] + rng.choice([c for c in "ACGT" if c != g[p + 1]]) + random_dna(rng, k + 1))
        for t in in_tips:  # a fresh k + 2 bases, then the backbone from offset t on: a source in front of fl + t
            p = fl + t
            seqs.append(random_dna(rng, k + 1) + rng.choice([c for c in "ACGT" if c != g[p - 1]]) + g[p:p + k + 1])
        if clean_haplotypes(seqs, k):
            break
    else:
        raise RuntimeError("bubble_ladder: no clean seed")
    true_len = n - 2 * fl
    gap = dict(left=g[:fl], right=g[n - fl:], gap_len=true_len + k, lmf=fuz, rmf=fuz, true_len=true_len)
    return dict(seqs=seqs, gap=gap, bubbles=bubbles, paths=(2 ** m if not indel else None))


# Planted gaps at the per-gap capacities of the fill kernels (k = 31, bubbles 32 bases apart, a seed of its own
# each, so that one graph can hold them all).  Each entry:
# bubble_ladder's arguments and what the gap is meant to give: the segments the left DP logs (`nseg`: the segment
# tier's log of G2S_SEG_CAP = 512, its 64-lane chunks, the 192 up to which the fill kernel analyses the closure
# itself), the right set's entries (`nA`: 64 * G2S_SEG_ASETS = 256), the closure's segments (`ncl`: g2s_d2_small
# takes 256) and phase C's path count (`count`, MAX_PATHS where absent).  tests/test_seg_model.py checks every value
# against the segment tier's model and the oracle; tests/test_gpu_edges.py checks that the kernels count the same and
# route the gap accordingly.  (3 segments a bubble + 2; an out-tip in the left half: +2 segments and +1 closure
# segment; an out-tip in the right half: +1 segment, +1 entry; an in-tip in the right half: +1 segment, +2 entries.)
_L = dict(k=31, spacing=32)
MAX_PATHS = 2147483647 // 2 - 1  # (Gap2Seq.cpp:38: 2^30 - 2, so 2^30 paths is the first count that saturates)
EDGE_LADDERS = {
    "seg63": (dict(_L, seed=101, m=20, tail=100, out_tips=(700,)), dict(nseg=63, nA=31, ncl=62, count=1 << 20)),
    "seg64": (dict(_L, seed=102, m=20, out_tips=(40,)), dict(nseg=64, nA=36, ncl=62, count=1 << 20)),
    "seg65": (dict(_L, seed=103, m=21), dict(nseg=65, nA=36, ncl=64, count=1 << 21)),
    "seg127": (dict(_L, seed=104, m=41, out_tips=(40,)), dict(nseg=127, nA=66, ncl=125)),
    "seg128": (dict(_L, seed=105, m=42), dict(nseg=128, nA=69, ncl=127)),
    "seg129": (dict(_L, seed=106, m=42, tail=100, out_tips=(1394,)), dict(nseg=129, nA=64, ncl=128)),
    "seg191": (dict(_L, seed=107, m=63), dict(nseg=191, nA=99, ncl=190)),
    "seg192": (dict(_L, seed=108, m=63, tail=100, out_tips=(2034,)), dict(nseg=192, nA=97, ncl=191)),
    "seg193": (dict(_L, seed=109, m=63, out_tips=(40,)), dict(nseg=193, nA=99, ncl=191)),
    "seg511": (dict(_L, seed=110, m=169, tail=5500, out_tips=(8000, 9000)), dict(nseg=511, nA=6, ncl=510)),
    "seg512": (dict(_L, seed=111, m=170, tail=5500), dict(nseg=512, nA=4, ncl=511)),
    "seg513": (dict(_L, seed=112, m=170, tail=5500, in_tips=(8440,)), dict(nseg=513, nA=6, ncl=512)),
    "rs255": (dict(_L, seed=113, m=83, lead=3000, tail=100, in_tips=(5706,)), dict(nseg=252, nA=255, ncl=251)),
    "rs256": (dict(_L, seed=114, m=84, lead=3000), dict(nseg=254, nA=256, ncl=253)),
    "rs257": (dict(_L, seed=115, m=84, lead=3000, tail=100, out_tips=(5706,)), dict(nseg=255, nA=257, ncl=254)),
    "cl255": (dict(_L, seed=116, m=84, out_tips=(40, 200)), dict(nseg=258, nA=132, ncl=255)),
    "cl256": (dict(_L, seed=117, m=85), dict(nseg=257, nA=132, ncl=256)),
    "cl257": (dict(_L, seed=118, m=85, out_tips=(40,)), dict(nseg=259, nA=132, ncl=257)),
    "paths2^29": (dict(_L, seed=119, m=29), dict(nseg=89, nA=48, ncl=88, count=1 << 29)),
    "paths2^30": (dict(_L, seed=120, m=30), dict(nseg=92, nA=51, ncl=91, count=MAX_PATHS)),
    "paths2^31": (dict(_L, seed=121, m=31), dict(nseg=95, nA=51, ncl=94, count=MAX_PATHS)),
    "indel20": (dict(_L, seed=122, m=20, indel=True), dict(nseg=239, nA=36, ncl=238, count=1 << 14)),
}


def edge_ladder(name):
    kw, want = EDGE_LADDERS[name]
    return bubble_ladder(**kw), want


def edge_ladder_list(names, pad=0):
    """The planted gaps of `names` as one list on one graph, among `pad` ordinary gaps of a plain genome (30 kbp,
    20-300 bp gaps): (haplotypes, gaps, index of each planted gap in the list).  The segment tier packs the closures
    of a list into one buffer of 64 segments a gap on average (g2s_api.hip, run_tier: a closure that finds it full
    runs again in the large variant); enough ordinary gaps keep the planted ones clear of that limit, so that the
    route of every gap is its own."""
    seqs, gaps, idx = [], [], []
    for name in names:
        lad, _ = edge_ladder(name)
        seqs += lad["seqs"]
        gaps.append(lad["gap"])
    if pad:
        genome = random_dna(SplitMix(909), 30000)
        seqs.append(genome)
        planted, gaps = gaps, cut_gaps(31, genome, 31, fuz=3, ngaps=pad, min_len=20, max_len=300, d_err=10, vary_fuz=False)
        for j, g in enumerate(planted):
            idx.append(min(len(gaps), 3 + 4 * j))
            gaps.insert(idx[-1], g)
    else:
        idx = list(range(len(gaps)))
    return seqs, gaps, idx


def scaffold_record(genome, k, fuz, pos_len_list, pad=5):
    """One multi-gap scaffold record: genome slice with N runs at the given
    (start, length, n_count) triples (sorted, non overlapping)."""
    lo = max(0, pos_len_list[0][0] - k - fuz - pad)
    hi = min(len(genome), pos_len_list[-1][0] + pos_len_list[-1][1] + k + fuz + pad)
    s = list(genome[lo:hi])
    out = []
    cur = lo
    for (p, ln, ncount) in pos_len_list:
        out.append(genome[cur:p])
        out.append("N" * ncount)
        cur = p + ln
    out.append(genome[cur:hi])
    return "".join(out)


def strand_flip_genome(seed, length, k, n=5, fuz=6):
    """Both strands of a k-mer at one depth (Q7) at any k: a genome with n hairpins (S + revcomp(S),
    |S| > k/2: a palindromic k-mer at even k) and a second haplotype with n inversions of k + 2r bases (the middle
    k-mer of an inversion and its reverse complement lie at the same depth from a seed in front of it).  Returns
    (haplotypes, gaps): the gaps of cut_gaps over the genome, then one gap across every hairpin and inversion."""
    rng = SplitMix(seed * 6151 + 5)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rc = lambda s: "".join(comp[c] for c in reversed(s))
    g = list(random_dna(rng, length))
    spots = []
    base = k + fuz + 40
    step = (length - base) // n  # (>= 2 (3k + 60) bases: a hairpin, then an inversion, each with its gap's flanks)
    for j in range(n):
        pos = base + j * step
        h = k // 2 + rng.randint(1, 8)
        s = random_dna(rng, h)
        g[pos:pos + 2 * h] = s + rc(s)
        spots.append((pos, pos + step // 2, k + 2 * rng.randint(2, 20)))
    g = "".join(g)
    h = g
    for pos, ipos, m in spots:
        h = h[:ipos] + rc(g[ipos:ipos + m]) + h[ipos + m:]
    gaps = cut_gaps(seed, g, k, fuz=fuz, ngaps=2 * n, min_len=5, max_len=80, d_err=k + 10)
    for pos, ipos, m in spots:
        for a, b in ((pos - 20, pos + k + 20), (ipos - 10, ipos + m + 10)):
            gaps.append(dict(left=g[a - k - fuz:a], right=g[b:b + k + fuz], gap_len=b - a + k, lmf=fuz, rmf=fuz,
                             true_len=b - a))
    return [g, h], gaps


BARELY_K, BARELY_SOLID = 5, 3


def barely_solid_reads(n_solid):
    """Reads for k = 5 at solid = 3 of which no k-mer (n_solid 0) or exactly one (n_solid 1) is solid: a text that holds
    every 5-mer over {A, C} once (none is another's reverse complement) as two reads, so a build finds 32 runs of two
    copies and has nothing to keep; and a third copy of one k-mer as a read of its own."""
    text = "AAAAACAAACCAACACAACCCACACCACCCCCAAAA"
    assert len({text[i:i + 5] for i in range(32)}) == 32 and set(text) == set("AC") and n_solid in (0, 1)
    return [text, text] + ["AACAC"] * n_solid
