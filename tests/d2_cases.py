"""tests/d2_cases.py — designed gaps whose closure has a known strong-component structure (phase D2,
/root/reference/src/Gap2Seq.cpp:1314-1435: gap2seq_amd/csrc/d2_device.hip on the device, post.cpp on the host).

Every design is ONE gap at k = 31, fuz 3, between random flanks of 200 bases; the gap is cut 100 bases inside them, so
that the closure starts and ends on plain text.  What lies between the flanks is written by hand from random units
(U, V, W of 50, 40 and 45 bases), random spacers (a .. d of 80 bases) and sub(s, p), s with base p substituted.  A
tandem array of a unit of u bases is a cycle of u k-mers in the graph (the unit's rotations), whatever the number of
copies; with -dist-error above the unit's length walks with fewer and with more turns than the text has fit the gap,
so the closure holds the cycle, each of its k-mers at several depths: the fill kernels leave such a closure to phase D2.

DESIGNS[name] = (builder, seed, d_err, want); `want` holds the designed values, checked against the oracle on the CPU
(tests/test_d2_cases.py) before any GPU run (tests/test_gpu_d2_designed.py):
  ncl     the closure's segments (tests/seg_model.py counts them): g2s_d2_small takes up to 256, g2s_d2_big the rest
  ncomp   nontrivial strong components of the closure (subgraph statistics [2])
  csize   their total size ([3]); None where it is only recorded
  count   the path count, where designed (MAX_PATHS: saturated)
  loop    True: the closure has a self loop on a trivial vertex, which is an edge and no component (edges == vertices)
  slow    True: oracle/pyref.py takes more than a few seconds (saturating counts through Python dicts)

A design whose haplotypes hold a k-mer that is its own reverse complement, or a k-mer whose reverse complement occurs
anywhere in them, is rejected and the next text of its stream is tried (strand_clean: repeats are allowed, unlike
cases.clean_haplotypes — these designs are made of them)."""
import cases

K, FUZ, FLANK, CUT = 31, 3, 200, 100
_COMP = str.maketrans("ACGT", "TGCA")


def sub(s, p):
    """s with base p substituted (by the next letter of ACGT)."""
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]


def kmers(seqs, k=K):
    return {s[i:i + k] for s in seqs for i in range(len(s) - k + 1)}


def strand_clean(seqs, k=K):
    """True when no k-mer of `seqs` is its own reverse complement and none meets its reverse complement anywhere in
    them (the oracle then sees no Q7 case and every field is compared)."""
    fwd = kmers(seqs, k)
    return not any(x.translate(_COMP)[::-1] in fwd for x in fwd)


def _units(rng):
    return dict(U=cases.random_dna(rng, 50), V=cases.random_dna(rng, 40), W=cases.random_dna(rng, 45),
                a=cases.random_dna(rng, 80), b=cases.random_dna(rng, 80), c=cases.random_dna(rng, 80),
                d=cases.random_dna(rng, 80))


def _ladder(rng, n):
    """L and L': n random bases and the same with a substitution every 32 (one bubble each, cases.bubble_ladder)."""
    L = cases.random_dna(rng, n)
    L2 = L
    for p in range(16, n, 32):
        L2 = sub(L2, p)
    return L, L2


# Builders: units -> (haplotypes between the flanks, where the gap begins in haplotype 0 relative to the left flank's
# end or None, where it ends relative to the right flank's start or None).  None: CUT bases inside the flank.
def _tandem(u, rng):
    return [u["a"] + u["U"] * 6 + u["b"]], None, None


def _tandem_short(u, rng):
    return [u["a"] + cases.random_dna(rng, 20) * 8 + u["b"]], None, None


def _two_cycle(u, rng):
    return [u["a"] + "AC" * 40 + u["b"]], None, None


def _self_loop(u, rng):
    return [u["a"] + "A" * 60 + u["b"]], None, None


def _series2(u, rng):
    return [u["a"] + u["U"] * 4 + u["b"] + u["V"] * 4 + u["c"]], None, None


def _series3(u, rng):
    return [u["a"] + u["U"] * 4 + u["b"] + u["V"] * 4 + u["c"] + u["W"] * 4 + u["d"]], None, None


def _parallel(u, rng):
    return [u["a"] + u["U"] * 4 + u["b"], sub(u["a"], 40) + u["V"] * 4 + u["b"]], None, None


def _chord(u, rng):
    U = u["U"]
    return [u["a"] + U * 5 + u["b"], u["a"] + U * 2 + sub(U, 25) + U * 2 + u["b"]], None, None


def _figure8(u, rng):
    X, Y, Z = cases.random_dna(rng, 45), cases.random_dna(rng, 45), u["V"]
    return [u["a"] + (X + Z + Y + Z) * 3 + u["b"]], None, None


def _loop_in_component(u, rng):
    # U' = U with A*40 inserted at 10.  The unit's 90 rotations hold the k-mer A*31 once for every window of the run of
    # A: a run of r bases leaves 90 - (r - 31) distinct k-mers.  The designed 80 is a run of 41: the U of this design
    # has an A on exactly one side of the insertion (any other U is rejected like an unclean one; a run of 40 gives 81).
    U = u["U"]
    if (U[9] == "A") + (U[10] == "A") != 1 or U[8] == "A" or U[11] == "A":
        return None
    return [u["a"] + (U[:10] + "A" * 40 + U[10:]) * 4 + u["b"]], None, None


def _holds_sinks(u, rng):
    # the right flank's k + fuz bases lie inside the array (in its sixth and seventh copy): the sink positions are
    # k-mers of the cycle
    return [u["a"] + u["U"] * 8 + u["b"]], None, 80 + 5 * 50 + 20


def _holds_source(u, rng):
    # the left flank's k + fuz bases lie inside the array (they end in its third copy): the seeds are k-mers of the cycle
    return [u["a"] + u["U"] * 8 + u["b"]], 80 + 2 * 50 + 20, None


def _two_depths(u, rng):
    return [u["a"] + u["U"] * 2 + u["b"]], None, None


def _cycle_bubbles(n):
    def build(u, rng):
        L, L2 = _ladder(rng, n)
        return [u["a"] + u["U"] * 4 + L + u["b"], u["a"] + u["U"] * 4 + L2 + u["b"]], None, None
    return build


MAX_PATHS = cases.MAX_PATHS
# (ncl is far above 3 segments a bubble or a turn wherever a k-mer is reached at many depths: every turn of a cycle that
# fits -dist-error enters what lies behind it at a depth of its own, and a 2-cycle or a loop fits hundreds of times.
# G2S_D2_LOG on an MI355X, ns = segments on paths to a sink: equal to ncl for every design; cycle+bubbles-90 has 1 911,
# its run graph 646 nodes and 736 edges.)
DESIGNS = {
    "tandem": (_tandem, 301, 200, dict(ncl=29, ncomp=1, csize=50)),
    "tandem-short-unit": (_tandem_short, 302, 200, dict(ncl=51, ncomp=1, csize=20)),
    "two-cycle": (_two_cycle, 303, 200, dict(ncl=378, ncomp=1, csize=2)),
    "self-loop": (_self_loop, 304, 200, dict(ncl=468, ncomp=0, csize=0, loop=True)),
    "series-2": (_series2, 305, 200, dict(ncl=149, ncomp=2, csize=90)),
    "series-3": (_series3, 306, 300, dict(ncl=596, ncomp=3, csize=135)),
    "parallel-arms": (_parallel, 307, 300, dict(ncl=90, ncomp=2, csize=90)),
    "chord": (_chord, 308, 200, dict(ncl=50, ncomp=1, csize=81)),  # (50 + the 31 k-mers of the chord)
    "figure-8": (_figure8, 309, 300, dict(ncl=50, ncomp=1, csize=None)),
    "loop-in-component": (_loop_in_component, 310, 300, dict(ncl=2758, ncomp=1, csize=80, count=MAX_PATHS, slow=True)),
    "cycle-holds-sinks": (_holds_sinks, 311, 200, dict(ncl=21, ncomp=1, csize=50)),
    "cycle-holds-source": (_holds_source, 312, 200, dict(ncl=29, ncomp=1, csize=50)),
    "one-path-two-depths": (_two_depths, 313, 40, dict(ncl=5, ncomp=1, csize=50, count=1)),
    "cycle+bubbles-30": (_cycle_bubbles(960), 314, 150, dict(ncl=651, ncomp=1, csize=50, count=MAX_PATHS)),
    "cycle+bubbles-90": (_cycle_bubbles(2880), 315, 150, dict(ncl=1911, ncomp=1, csize=50, count=MAX_PATHS)),
}
NAMES = list(DESIGNS)
D_ERRS = sorted({v[2] for v in DESIGNS.values()})
_BUILT = {}


def design(name):
    """dict(seqs, gap, d_err, want) of one design; seqs[0] is the haplotype the gap is cut from."""
    if name in _BUILT:
        return _BUILT[name]
    build, seed, d_err, want = DESIGNS[name]
    rng = cases.SplitMix(seed * 6151 + 211)
    for _ in range(1000):
        left, right = cases.random_dna(rng, FLANK), cases.random_dna(rng, FLANK)
        made = build(_units(rng), rng)
        if made is None:
            continue
        mids, begin, end = made
        seqs = [left + m + right for m in mids]
        if strand_clean(seqs):
            break
    else:
        raise RuntimeError("d2_cases: no clean text for " + name)
    g = seqs[0]
    a = CUT if begin is None else FLANK + begin
    b = len(g) - FLANK + CUT if end is None else FLANK + end
    gap = dict(left=g[a - K - FUZ:a], right=g[b:b + K + FUZ], gap_len=b - a + K, lmf=FUZ, rmf=FUZ, true_len=b - a)
    _BUILT[name] = dict(seqs=seqs, gap=gap, d_err=d_err, want=want)
    return _BUILT[name]


def takes_big(name):
    """The closure has more segments than g2s_d2_small holds (G2S_D2_SMALL_NS)."""
    return DESIGNS[name][3]["ncl"] > 256


def names_at(d_err):
    return [n for n in NAMES if DESIGNS[n][2] == d_err]


def design_list(d_err, pad=100):
    """The designs of one -dist-error as one list on one graph, among `pad` ordinary gaps of a plain genome, as
    cases.edge_ladder_list plants its ladders: (haplotypes, gaps, index of each design's gap, the designs' names)."""
    names = names_at(d_err)
    seqs, gaps, idx = [], [], []
    for n in names:
        d = design(n)
        seqs += d["seqs"]
        gaps.append(d["gap"])
    if pad:
        genome = cases.random_dna(cases.SplitMix(911 + d_err), 30000)
        seqs.append(genome)
        planted, gaps = gaps, cases.cut_gaps(37, genome, K, fuz=FUZ, ngaps=pad, min_len=20, max_len=300, d_err=10, vary_fuz=False)
        for j, g in enumerate(planted):
            idx.append(min(len(gaps), 3 + 4 * j))
            gaps.insert(idx[-1], g)
    else:
        idx = list(range(len(gaps)))
    return seqs, gaps, idx, names
