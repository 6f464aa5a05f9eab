"""Workloads and the brute-force model of the single-graph build bounded by reach records (g2s_graph_build_seqs_reach,
g2s_graph_build_files_reach), shared by tests/test_graph_reach.py (host build) and tests/test_gpu_graph_reach.py (device
build).

The model is reach_cases' (written from the definition in include/g2s.h, no code shared with the product) extended to
many records with their own radii: every record's ball is searched on its own, breadth first over the eight possible
neighbours of a canonical k-mer, and the kept set is the union of the balls."""
import cases
import reach_cases as RC

KS = [4, 5, 31, 32, 33, 63, 64, 65]


def gap_obj(P, g):
    return P.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"])


def reach_of(P, records):
    return [(gap_obj(P, g), r) for g, r in records]


def ball(full, seeds, radius):
    kept = {x for x in seeds if x in full}
    frontier, level = sorted(kept), 0
    while frontier and level < radius:
        nxt = []
        for x in frontier:
            for y in RC.neighbours(x):
                if y in full and y not in kept:
                    kept.add(y)
                    nxt.append(y)
        frontier, level = nxt, level + 1
    return kept


def model(seqs, records, k, solid):
    """(full, kept) for records = [(gap dict, radius)]"""
    counts = RC.kmer_counts(seqs, k)
    full = {x for x, c in counts.items() if c >= max(1, solid)}
    kept = set()
    for g, radius in records:
        kept |= ball(full, RC.seeds_of(g, k), radius)
    return full, kept


def assert_matches_model(P, u, full, kept, outside=()):
    """graph u against the model: the k-mers (count, membership of every k-mer of the full set and of `outside`) and the
    successors of every kept node on both strands"""
    assert u.num_sets == 1 and u.num_kmers == len(kept), "%d k-mers, the model keeps %d of %d" % (u.num_kmers, len(kept), len(full))
    for x in list(full) + [RC.canon(y) for y in outside]:
        v = u.node(x)
        assert (v != P.G2S_INVALID_NODE) == (x in kept), x
        if x in kept:
            assert sorted(u.node_string(w) for w in u.successors(v)) == RC.successors(u.node_string(v), kept), x
            if RC._rc(x) == x:   # a palindrome (even k) exists on one strand only
                assert u.successors(v ^ 1) == []
                continue
            assert sorted(u.node_string(w) for w in u.successors(v ^ 1)) == RC.successors(u.node_string(v ^ 1), kept), x
    assert u.validate() == (0, "")


def view(u):
    """a graph up to the numbering of its nodes: every oriented node's string with its successors' strings"""
    out = {}
    for v in range(2 * u.num_kmers):
        out[u.node_string(v)] = sorted(u.node_string(w) for w in u.successors(v))
    return out


def assert_same_graph(a, b):
    assert a.num_kmers == b.num_kmers and a.num_unitigs == b.num_unitigs
    assert view(a) == view(b)
    assert a.validate() == (0, "") and b.validate() == (0, "")


def workload(k, solid):
    """(seqs, gaps): reads (every one `solid` times) and named gaps.
      A, B   gaps of the main read 60 bases apart (5 at small k): their balls overlap;
      C      a gap of the main read far from both;
      E      a gap of the island, a short read that is a component of its own: a search from it dies out early;
      D      a gap whose flanks are in no read.
    Unrelated reads keep every bounded graph a proper part of the full one."""
    small = k < 11
    rng = cases.SplitMix(900 + k)
    if small:
        main = cases.one_strand_genome(50 + k, 300, "AC")  # dense: 2^k possible k-mers
        island = RC._no_runs(rng, 44, "AT", k)
        unrelated = [RC._no_runs(rng, 60, "AG", k)]
        absent = RC._no_runs(rng, 4 * k + 30, "CG", k)
        gl, lmf, rmf, apart = 6, 1, 1, 5
    else:
        gl, lmf, rmf, apart = 30, 3, 2, 60
        main = cases.random_dna(rng, 2600)
        island = cases.random_dna(rng, 2 * k + lmf + rmf + gl + 12)
        unrelated = [cases.random_dna(rng, 300) for _ in range(2)]
        absent = cases.random_dna(rng, 4 * k + 40)

    def gap_at(text, pos):
        return dict(left=text[pos - k - lmf:pos], right=text[pos + gl:pos + gl + k + rmf], gap_len=gl + k, lmf=lmf, rmf=rmf)
    first = k + lmf + 40 if not small else k + lmf + 10
    gaps = dict(A=gap_at(main, first), B=gap_at(main, first + apart), C=gap_at(main, len(main) - 2 * k - gl - 60),
                E=gap_at(island, k + lmf + 4), D=gap_at(absent, k + lmf + 2))
    seqs = []
    for s in [main, island] + unrelated:
        seqs += [s] * solid
    return seqs, gaps


def scenarios(k, gaps):
    """name -> records: the cases of the issue.  `late` enters C at level 145 (12 at small k) of a search that E's
    island has long ended; `twice` names one gap with both radii: the larger must win."""
    small = k < 11
    deep, late = (4, 2) if small else (150, 5)
    return {
        "radius0": [(gaps["A"], 0)],
        "radius1": [(gaps["A"], 1)],
        "staggered": [(gaps["A"], 3), (gaps["B"], 2 if small else 40)],
        "twice": [(gaps["A"], 0 if small else 3), (gaps["A"], 2 if small else 40)],
        "late": [(gaps["E"], deep + (10 if small else 0)), (gaps["C"], late)],
        "absent_seed": [(gaps["A"], 1 if small else 5), (gaps["D"], 5)],
    }


def palindrome_case(k, r, seed=2):
    """(seqs, gap): one read in which a palindromic k-mer (even k) starts r bases behind the right flank's k-mer, so that
    it lies on the rim of the ball of radius r (the caller checks that with the model); a second read keeps the graph
    a proper part of the full one"""
    assert k % 2 == 0
    rng = cases.SplitMix(seed * 100 + k)
    w = cases.random_dna(rng, k // 2)
    pal = w + RC._rc(w)
    gl = 10
    pre = cases.random_dna(rng, r + gl + k + 8)
    read = pre + pal + cases.random_dna(rng, 3 * k + 20)
    q = len(pre)
    gap = dict(left=read[q - r - gl - k:q - r - gl], right=read[q - r:q - r + k], gap_len=gl + k, lmf=0, rmf=0)
    return [read, cases.random_dna(rng, 200 if k > 10 else 12)], gap, pal
