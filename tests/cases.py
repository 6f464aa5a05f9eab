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


def bubble_ladder(seed, k, m, spacing, indel=False, lead=0, tail=0, out_tips=(), in_tips=(), fuz=3, indel_every=3,
                  run=0, run_step=None, del_len=1):
    """A chain of m bubbles between two flanks, with tips added on demand.  Returns dict(seqs, gap, bubbles, paths):
    seqs[0] is the random backbone, seqs[1] a second haplotype with m substitutions `spacing` (>= k + 1) bases apart,
    the first `lead` bases after the left flank's last k-mer and the last `tail` bases in front of the right flank's
    first k-mer; gap is the cut_gaps-style record of the one gap from the backbone's first k + fuz bases to its last.

    Closure shape (k-mers, not bases): every substitution gives a bubble of two arms of k k-mers each; between two
    bubbles the haplotypes share spacing - k k-mers, one unitig.  The left DP therefore logs one segment per arm and
    one per shared stretch: about 3 segments per bubble, 2^m paths of one length (the count saturates at MAX_PATHS
    from m = 30 on).  With indel=True every third bubble is a deletion on haplotype 2 instead (arms of k and k - 1
    k-mers): later unitigs are entered at two depths, the paths have several lengths, and the closure has k-mers at
    several depths (the fill kernels leave it to phase D2 on the device or to the host).  indel_every = n makes every
    n-th bubble the deletion instead: behind d deletions a unitig is entered at d + 1 depths, so the logged segments
    grow with the square of their number (a substitution ladder logs 3 a bubble and would need D > 32767 to fill the
    large variant's log at k = 31).

    out_tips: backbone offsets (from the left flank's last k-mer) at which a dead end of k + 2 bases branches off
    (a third read that leaves the backbone): in the left half of the gap each cuts one unitig in two and adds the
    tip's own segment: +2 logged segments, no right-set entry.  in_tips: offsets at which a source of k + 2 bases
    joins the backbone (a read that ends on it): the backbone's unitig is cut (+1 logged segment) and the tip is
    one more predecessor for phase A to enter (+1 right-set entry when it lies in the right half).  Seeds whose
    haplotypes repeat a k-mer anywhere (either strand) are rejected and the next seed of the stream is tried.

    run = J (tests/trace_cases.py): every substitution becomes a row of them, run_step (<= k - 1, default k - 1) bases
    apart over J bases: the arms do not meet between two of them, so the bubble's arms are J' + k k-mers long (J' the
    distance from the first to the last substitution) — a run of unsafe states longer than a wave.  del_len = n: a
    deletion takes n bases (arms of k and k - n k-mers: paths whose lengths differ by n; two lengths are both phase
    C's only when they differ by an even number, :1125-1126).  lead may be negative (down to 1 - fuz): the first
    bubble then opens inside the left seeds.  With the defaults the output is what it was without these arguments."""
    assert spacing >= k + 1 + run and del_len >= 1
    rng = SplitMix(seed * 6151 + 101)
    fl = k + fuz
    n = fl + lead + (m - 1) * spacing + 1 + tail + fl if m else fl + lead + tail + fl
    n += (run + del_len - 1) if m else 0
    step = run_step or k - 1
    assert 1 <= step <= k - 1
    for _ in range(1000):
        g = random_dna(rng, n)
        h = list(g)
        bubbles = []
        for b in range(m):
            p = fl + lead + b * spacing
            if indel and b % indel_every == indel_every - 1:
                for q in range(del_len):
                    h[p + q] = ""
            else:
                for q in range(0, run + 1, step):
                    h[p + q] = "ACGT"[("ACGT".index(h[p + q]) + 1 + rng.randint(0, 2)) % 4]
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


def fan_paths(widths):
    """The leaves of a tree of free bases with widths[j] nodes at level j + 1, as strings over ACGT: child c of a level
    hangs from node c mod (nodes above) and takes the base c div (nodes above), so every node has two to four children
    (a node with one child would be no branch: the unitig would go on) and widths sets each level to the unit."""
    level = [""]
    for w in widths:
        assert 2 * len(level) <= w <= 4 * len(level), widths
        level = [level[c % len(level)] + "ACGT"[c // len(level)] for c in range(w)]
    return level


def _numbered_along(read, k, n):
    """Does the k-mer index grow along `read` over its first n k-mers, taken as one unitig?  The graph numbers a unitig
    in the direction in which its smallest canonical k-mer (bases ordered A, C, T, G) reads canonically (dbg.cpp,
    unitig_order)."""
    order = str.maketrans("ACGT", "0132")
    comp = str.maketrans("ACGT", "TGCA")
    best = None
    for i in range(n):
        x = read[i:i + k]
        f, r = x.translate(order), x.translate(comp)[::-1].translate(order)
        c = (min(f, r), f <= r)
        if best is None or c < best:
            best = c
    return best[1]


def fan_trees(seed, k, out=(), inn=(), link=1, lead=20, mid=40, tail=20, leaf_out=8, leaf_in=100, merge=False, fuz=3,
              aligned=False):
    """One gap whose left flank opens into a fan-out tree and whose right flank is reached through a fan-in tree.
    Returns dict(seqs, gap) as bubble_ladder does; seqs[0] is the backbone, the one read from flank to flank.

    out: the fan-out trees, a list of (spacer, widths).  Behind the left flank and `lead` shared bases the reads differ
    in consecutive free bases (fan_paths(widths)): the k-mers that end on the j-th free base are the widths[j - 1]
    events of one round of phase B, each a unitig of one k-mer, so widths[-1] events are pending behind the last
    level.  With several trees the root has one child per tree (one more free base), and tree t begins behind `spacer`
    bases of its own: a longer spacer puts the subtree deeper, where its events wait while the others run.  A leaf
    ends after leaf_out more bases (a dead end) unless it is linked.  merge: two more reads leave node 0 of the last
    level but two one level early, differ in that one base and share what follows: two arms of k k-mers, final in
    the same round as the last level's parents, whose one child is proposed twice in that round (a merge).
    inn: the widths of the fan-in tree, the mirror image in front of the right flank and `tail` shared bases: a leaf
    is a read of leaf_in bases that joins through its free bases.  Phase A enters every leaf; where leaf_in is longer
    than what right_half still reaches it stops inside, so that the right set's intervals keep holes between them.
    aligned: every leaf of `inn` is drawn again until its unitig is numbered along the read.  Phase A covers the end
    of a leaf; of two leaves numbered one after the other in opposite directions the covered ends can touch and their
    intervals merge (a quarter of all pairs): with every leaf numbered the same way M stays near the number of leaves,
    which M = 4097 needs to fit below G2S_SEGX_EA entries (an entry per leaf and one per node of the tree).
    link: leaves 0 .. link - 1 of out[0] run on, through `mid` bases of their own, into the same leaves of `inn` (the
    backbone is leaf 0; without a tree on a side the backbone simply has no free bases there)."""
    rng = SplitMix(seed * 6151 + 211)
    fl = k + fuz
    opaths = [(t, p) for t, (_, widths) in enumerate(out) for p in fan_paths(widths)] or [(0, "")]
    ipaths = fan_paths(inn) if inn else [""]
    n0 = len(fan_paths(out[0][1])) if out else 1
    assert 1 <= link <= min(n0, len(ipaths))
    for _ in range(1000):
        pre, post = random_dna(rng, fl + lead), random_dna(rng, tail + fl)
        stems = [("ACGT"[t] if len(out) > 1 else "") + random_dna(rng, sp) for t, (sp, _) in enumerate(out)] or [""]
        seqs = []
        for i, (t, p) in enumerate(opaths):
            head = (pre if i == 0 else pre[1 - k:]) + stems[t] + p
            if i < link:
                seqs.append(head + random_dna(rng, mid) + ipaths[i][::-1] + (post if i == 0 else post[:k - 1]))
            else:
                seqs.append(head + random_dna(rng, leaf_out))
        for p in ipaths[link:]:
            while True:
                seqs.append(random_dna(rng, leaf_in) + p[::-1] + post[:k - 1])
                if not aligned or _numbered_along(seqs[-1], k, leaf_in):
                    break
                seqs.pop()
        if merge:
            widths = out[0][1]
            assert len(out) == 1 and len(widths) >= 3 and widths[-2] <= 2 * widths[-3]
            arm = random_dna(rng, k + leaf_out)
            stem = pre[1 - k:] + stems[0] + fan_paths(widths[:-2])[0]
            seqs += [stem + "G" + arm, stem + "T" + arm]
        if clean_haplotypes(seqs, k):
            break
    else:
        raise RuntimeError("fan_trees: no clean seed")
    g = seqs[0]
    true_len = len(g) - 2 * fl
    gap = dict(left=g[:fl], right=g[len(g) - fl:], gap_len=true_len + k, lmf=fuz, rmf=fuz, true_len=true_len)
    return dict(seqs=seqs, gap=gap)


# Planted gaps at the limits behind EDGE_LADDERS that bubble ladders do not reach (k = 31, d_err 10), a graph of its own
# each.  Each entry: the generator ("fan": fan_trees, "ladder": bubble_ladder), its arguments and what the gap gives by
# the model (tests/seg_model.py): `nseg`, `nA`, `ncl`, `count` as in EDGE_LADDERS; `ev`: the most events pending behind
# a round (g2s_fill_seg / g2s_fill_seg2 hold 64: WHY_FRONTIER from 65 on); `ring`: the most, over the rounds, of events
# pending at the round's start plus children proposed in it (g2s_fill_segw's ring hands out G2S_SEGX_PE = 1024 slots a
# round: WHY_FRONTIER from 1025 on); `gen`: the rounds of phase B (the dump's roundsB); where given, `merges`: children
# of the fullest round that met their event pending, `sweeps`: rebuilds of the large variant's event table with events
# live, `M`: merged intervals of the right set.  tests/test_seg_model.py proves every value and the model's equality
# with the oracle; tests/test_gpu_segw_edges.py checks that the kernels count and route the same.
_F = dict(k=31, lead=20, tail=200)
FRONTIER_EDGES = {
    # the regular tier's 64 lanes: 63 / 64 / 65 events behind the round of the tree's last level
    "ev63": ("fan", dict(_F, seed=301, out=[(0, (4, 16, 63))]), dict(nseg=85, nA=4, ncl=4, count=1, ev=63, ring=79, gen=5)),
    "ev64": ("fan", dict(_F, seed=302, out=[(0, (4, 16, 64))]), dict(nseg=86, nA=4, ncl=4, count=1, ev=64, ring=80, gen=5)),
    "ev65": ("fan", dict(_F, seed=303, out=[(0, (4, 8, 17, 65))]),
             dict(nseg=96, nA=4, ncl=5, count=1, ev=65, ring=82, gen=6)),
    # 63 new events and the arms' child, proposed twice: 64 pending and a 65th child that merges
    "ev64merge": ("fan", dict(_F, seed=304, out=[(0, (4, 8, 16, 63))], merge=True),
                  dict(nseg=96, nA=4, ncl=5, count=1, ev=64, ring=83, gen=7, merges=1)),
    # 64 leaves that all reach the right flank, the last level's children at depth prune_from exactly: the round
    # that fills the lanes is the first to need the right set (two waves: the round that starts again)
    "ev64straddle": ("fan", dict(k=31, seed=305, out=[(0, (4, 16, 64))], inn=(4, 16, 64), link=64, mid=40, tail=10, lead=91),
                     dict(nseg=107, nA=109, ncl=106, count=64, ev=64, ring=128, gen=8, straddle=True)),
    # the large variant's ring: 256 events pending and 768 / 769 children; once with a subtree of 855 events run
    # and dead before (one sweep of the event table, four events live)
    "ring1024": ("fan", dict(_F, seed=306, out=[(0, (4, 16, 64, 256, 768))]),
                 dict(nseg=1110, nA=4, ncl=6, count=1, ev=768, ring=1024, gen=7, sweeps=0)),
    "ring1025": ("fan", dict(_F, seed=307, out=[(0, (4, 16, 64, 256, 769))]),
                 dict(nseg=1111, nA=4, ncl=6, count=1, ev=769, ring=1025, gen=7)),
    "ring1024sweep": ("fan", dict(_F, seed=308, out=[(30, (4, 16, 64, 256, 768)), (0, (4, 16, 64, 256, 512))]),
                      dict(nseg=1964, nA=4, ncl=7, count=1, ev=768, ring=1024, gen=13, sweeps=1)),
}
_LOG = dict(k=31, spacing=32, seed=611, indel=True, indel_every=2, lead=200, m=146)
_RS = dict(k=31, lead=20, tail=10, mid=20, leaf_in=50, seed=621)
_IV = dict(k=31, lead=70, tail=10, mid=10, leaf_in=80, leaf_out=30, out=[(0, (4, 16, 64))], aligned=True)
SEGW_EDGES = {
    # G2S_SEGX_CAP = 16384 logged segments: 146 bubbles, every second a deletion, D = 4888; 31 sweeps of the event table
    "log16383": ("ladder", dict(_LOG, out_tips=(2424, 1176)),
                 dict(nseg=16383, nA=238, ncl=5204, ev=81, ring=107, gen=3245, sweeps=31)),
    "log16384": ("ladder", dict(_LOG, out_tips=(2424, 1176), in_tips=(120,)),
                 dict(nseg=16384, nA=238, ncl=5205, ev=81, ring=107, gen=3246, sweeps=31)),
    "log16385": ("ladder", dict(_LOG, out_tips=(2424, 1176, 90)),
                 dict(nseg=16385, nA=238, ncl=5205, ev=81, ring=107, gen=3246, sweeps=31)),
    # G2S_SEGX_EA = 6144 right-set entries: a fan-in tree of 4603 / 4604 leaves (and one more node inside)
    "rs6143": ("fan", dict(_RS, inn=(2, 5, 18, 72, 288, 1151, 4603)), dict(nseg=9, nA=6143, ncl=8, count=1, ev=1, ring=2, gen=9)),
    "rs6144": ("fan", dict(_RS, inn=(2, 5, 18, 72, 288, 1151, 4604)), dict(nseg=9, nA=6144, ncl=8, count=1, ev=1, ring=2, gen=9)),
    "rs6145": ("fan", dict(_RS, inn=(2, 5, 18, 72, 288, 1152, 4604)), dict(nseg=9, nA=6145, ncl=8, count=1, ev=1, ring=2, gen=9)),
    # the levels of the right set's search (iv_rank reads one more when M passes 8, 64, 512, 4096): M depends on the
    # numbering of the unitigs, so these graphs are built on the host (G2S_HOST_BUILD=1), one graph a gap
    "iv8": ("fan", dict(_IV, seed=403, inn=(4,), link=2), dict(nseg=9, nA=13, ncl=8, count=2, ev=2, ring=4, gen=6, M=8)),
    "iv9": ("fan", dict(_IV, seed=421, inn=(4,), link=2), dict(nseg=9, nA=13, ncl=8, count=2, ev=2, ring=4, gen=6, M=9)),
    "iv64": ("fan", dict(_IV, seed=441, inn=(2, 5, 19, 73), link=16),
             dict(nseg=62, nA=124, ncl=61, count=16, ev=16, ring=32, gen=9, M=64)),
    "iv65": ("fan", dict(_IV, seed=461, inn=(2, 5, 20, 77), link=16),
             dict(nseg=62, nA=129, ncl=61, count=16, ev=16, ring=32, gen=9, M=65)),
    "iv512": ("fan", dict(_IV, seed=481, inn=(3, 9, 34, 134, 536), link=32),
              dict(nseg=131, nA=741, ncl=130, count=32, ev=32, ring=64, gen=10, M=512)),
    "iv513": ("fan", dict(_IV, seed=501, inn=(3, 9, 34, 134, 534), link=32),
              dict(nseg=131, nA=739, ncl=130, count=32, ev=32, ring=64, gen=10, M=513)),
    "iv4096": ("fan", dict(_IV, seed=560, inn=(2, 5, 17, 65, 258, 1031, 4123), link=32),
               dict(nseg=175, nA=5526, ncl=174, count=32, ev=32, ring=64, gen=12, M=4096)),
    "iv4097": ("fan", dict(_IV, seed=580, inn=(2, 5, 17, 65, 258, 1032, 4128), link=32),
               dict(nseg=175, nA=5532, ncl=174, count=32, ev=32, ring=64, gen=12, M=4097)),
}
LIMIT_EDGES = dict(FRONTIER_EDGES, **SEGW_EDGES)
_limit_cache = {}


def limit_edge(name):
    """(dict(seqs, gap), want) of one row of FRONTIER_EDGES / SEGW_EDGES; built once a process."""
    if name not in _limit_cache:
        how, kw, _ = LIMIT_EDGES[name]
        _limit_cache[name] = bubble_ladder(**kw) if how == "ladder" else fan_trees(**kw)
    return _limit_cache[name], LIMIT_EDGES[name][2]


def limit_edge_list(names, pad=0):
    """edge_ladder_list for rows of FRONTIER_EDGES / SEGW_EDGES: (haplotypes, gaps, index of each planted gap)."""
    seqs, gaps, idx = [], [], []
    for name in names:
        lad, _ = limit_edge(name)
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
