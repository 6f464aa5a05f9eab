"""Workloads and comparisons of the pooled set build (g2s_graph_build_pool) shared by tests/test_read_pool.py (host
build) and tests/test_gpu_read_pool.py (device build): sets given as index lists into one pool of sequences, plus a
shared list, against g2s_graph_build_sets on the expanded lists, set by set."""
import cases
from gap2seq_amd import lib as P


def pool_workload(k, shared_mode="shared"):
    """(seqs, set_lists, shared, set_shared) with: a sequence in several sets, and twice in one set, where a k-mer is
    solid at 2 only through the duplicate (A in set 0); a k-mer once in a set's own reads and once in the shared list
    (X: set 1 flagged, set 2 the same own reads unflagged); a k-mer solid in the shared list alone (D, twice there);
    an own-only solid k-mer in a flagged set (E in set 1); a flagged set with no own reads (3); an empty unflagged set
    (4); sets with a circular unitig (5, and 6 flagged); a read shorter than k (7).
    shared_mode: "shared" | "empty" (flags set, the shared list empty) | "none" (set_shared None)."""
    rng = cases.SplitMix(900 + k)
    g = cases.random_dna(rng, 1500)
    unit = cases.random_dna(rng, k + 19)
    a, b, c, e = g[0:400], g[300:700], g[650:1000], g[1000:1300]
    d, x = cases.random_dna(rng, 300), cases.random_dna(rng, 250)
    seqs = [a, b, c, d, e, unit * 4, x, g[:k - 1]]
    A, B, Cq, D, E, TAN, X, SHORT = range(8)
    set_lists = [[A, A, B], [A, B, X, E, E], [A, B, X, E, E], [], [], [TAN, TAN], [TAN, Cq, TAN, Cq], [SHORT], [A]]
    set_shared = [0, 1, 0, 1, 0, 0, 1, 0, 1]
    shared = [D, D, X]
    if shared_mode == "empty":
        shared = []
    elif shared_mode == "none":
        set_shared = None
    return seqs, set_lists, shared, set_shared


def expanded(seqs, set_lists, shared, set_shared):
    return [[seqs[i] for i in own] + ([seqs[i] for i in shared] if set_shared is not None and set_shared[s] else [])
            for s, own in enumerate(set_lists)]


def canon(x):
    rc = x.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    code = str.maketrans("ACTG", "0123")  # GATB codec order A0 C1 T2 G3
    return min(x, rc, key=lambda y: y.translate(code))


def set_view(u, s):
    """set s of a set graph as strings: {k-mer: (successors of both orientations, as strings)}"""
    first, cnt = u.set_nodes(s)
    out = {}
    for i in range(first, first + cnt):
        x = canon(u.node_string(2 * i))  # (orientations are unitig-relative: the canonical string names the k-mer)
        v = u.set_node(s, x)
        assert v >> 1 == i and u.node_string(v) == x
        for w in u.successors(v) + u.successors(v ^ 1):
            assert first <= w >> 1 < first + cnt, "edge out of set %d" % s
        out[x] = ([u.node_string(w) for w in u.successors(v)], [u.node_string(w) for w in u.successors(v ^ 1)])
    return out


def assert_same_graph(pool, sets, nsets):
    assert pool.num_sets == sets.num_sets == nsets
    assert pool.num_kmers == sets.num_kmers and pool.num_unitigs == sets.num_unitigs
    for s in range(nsets):
        assert pool.set_nodes(s) == sets.set_nodes(s), "set %d" % s
        assert set_view(pool, s) == set_view(sets, s), "set %d" % s
    assert pool.validate() == (0, "")


def assert_workload_properties(u, seqs, k, solid, shared_mode):
    """the cases the workload exists for, read off the graph"""
    a, b, d, e, x = seqs[0], seqs[1], seqs[3], seqs[4], seqs[6]
    absent = P.G2S_INVALID_NODE
    assert u.set_nodes(4)[1] == 0 and u.set_nodes(7)[1] == 0
    assert u.set_node(0, a[:k]) != absent            # A twice in set 0 ...
    assert (u.set_node(8, a[:k]) == absent) == (solid == 2)  # ... and once in set 8
    assert (u.set_node(0, b[-k:]) == absent) == (solid == 2)  # B once in set 0; A counts through its duplicate
    assert u.set_node(1, e[:k]) != absent and u.set_node(2, e[:k]) != absent
    if shared_mode == "shared":
        assert u.set_node(1, x[:k]) != absent                  # once own + once shared
        assert (u.set_node(2, x[:k]) == absent) == (solid == 2)  # the same own reads, not flagged
        assert u.set_node(3, d[:k]) != absent and u.set_node(1, d[:k]) != absent and u.set_node(2, d[:k]) == absent
        assert (u.set_node(3, x[:k]) == absent) == (solid == 2)  # once in the shared list alone
    else:
        assert u.set_nodes(3)[1] == 0 and u.set_node(1, d[:k]) == absent
        assert u.set_nodes(1)[1] == u.set_nodes(2)[1]
    assert u.set_nodes(5)[1] == k + 19                         # the tandem read: one circular unitig


D_ERR = 100
FUZ = 10


def fill_workload(k, seed, ngaps, flag=lambda s: s % 3 == 0):
    """(seqs, set_lists, shared, set_shared, gaps, gap_set) for a list of gaps filled set by set: one set a gap. A set
    without the flag holds windows of both haplotypes around its gap and a window from elsewhere; a flagged set holds
    the second haplotype's window alone as its own reads and gets the first haplotype from the shared list, tiles of
    the whole genome, so its fill depends on the shared reads. The windows overlap: the pool holds every distinct
    read once. The last two sets have no own reads (one flagged, one not); each is named by a copy of the first gap."""
    hap = cases.toy_genome(seed, 12000, k, repeats=6, tandem=2, snp_every=350)
    genome = hap[0]
    rng = cases.SplitMix(seed * 31 + k)
    raw = cases.cut_gaps(seed, genome, k, FUZ, ngaps, 10, 160, D_ERR)
    seqs, index = [], {}

    def entry(text):
        if text not in index:
            index[text] = len(seqs)
            seqs.append(text)
        return index[text]
    set_lists, set_shared, gaps, gap_set = [], [], [], []
    for s, g in enumerate(raw):
        pos = genome.find(g["left"]) + len(g["left"])
        lo, hi = max(0, pos - 150), min(len(genome), pos + g["true_len"] + 150)
        o = rng.randint(0, len(genome) - 400)
        if flag(s):
            set_lists.append([entry(hap[1][lo:hi])])
        else:
            set_lists.append([entry(h[lo:hi]) for h in hap] + [entry(genome[o:o + 400])])
        set_shared.append(1 if flag(s) else 0)
        gaps.append(g)
        gap_set.append(s)
    for flagged in (1, 0):
        set_lists.append([])
        set_shared.append(flagged)
        gaps.append(dict(raw[0]))
        gap_set.append(len(set_lists) - 1)
    shared = [entry(genome[j:j + 1000]) for j in range(0, len(genome) - 200, 800)]
    return seqs, set_lists, shared, set_shared, gaps, gap_set
