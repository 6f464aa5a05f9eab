"""Workloads and the brute-force model of the pooled set build with reach records (g2s_graph_build_pool_reach), shared
by tests/test_pool_reach.py (host build) and tests/test_gpu_pool_reach.py (device build).

The model is written from the definition in include/g2s.h and shares no code with the product: a dictionary of
canonical k-mers with their copies, the seeds as the fill's flank k-mers, a breadth-first search over the eight
possible neighbours of a k-mer."""
import cases

ORDER = "ACTG"  # GATB codes A0 C1 T2 G3


def _code(c):
    return (ord(c) >> 1) & 3


def _invalid(c):
    return (ord(c) >> 3) & 1


def _rc(x):
    return "".join(ORDER[_code(c) ^ 2] for c in reversed(x))


def canon(x):
    """the canonical k-mer of k characters, every byte mapped to some base as the fill's look-ups map it"""
    f = "".join(ORDER[_code(c)] for c in x)
    r = _rc(f)
    return min(f, r, key=lambda y: [_code(c) for c in y])


def kmer_counts(seqs, k):
    out = {}
    for s in seqs:
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if any(_invalid(c) for c in w):
                continue
            c = canon(w)
            out[c] = out.get(c, 0) + 1
    return out


def neighbours(x):
    out = []
    for f in (x, _rc(x)):
        for c in ORDER:
            out.append(canon(f[1:] + c))
    return out


def seeds_of(gap, k):
    """the flank k-mers the fill looks up; none for a gap it rejects"""
    if gap is None:
        return []
    left, right, lmf, rmf = gap["left"], gap["right"], gap["lmf"], gap["rmf"]
    if lmf < 0 or rmf < 0 or gap["gap_len"] < 0 or len(left) < k + lmf or len(right) < k + rmf:
        return []
    out = [left[x:x + k] for x in range(lmf + 1)]
    out += [right[len(right) - k - x:len(right) - x] for x in range(rmf + 1)]
    out += [right[x:x + k] for x in range(rmf + 1)]
    return [canon(s) for s in out]


def model_set(seqs, own, shared, flagged, gap, radius, k, solid):
    """(full, kept, levels): the set's full graph, what a reach record (gap, radius) keeps of it (radius None or < 0:
    all of it), and the deepest level the search reached"""
    counts = kmer_counts([seqs[i] for i in own] + ([seqs[i] for i in shared] if flagged else []), k)
    full = {x for x, c in counts.items() if c >= max(1, solid)}
    if radius is None or radius < 0:
        return full, set(full), 0
    kept = {x for x in seeds_of(gap, k) if x in full}
    frontier, level = sorted(kept), 0
    while frontier and level < radius:
        nxt = []
        for x in frontier:
            for y in neighbours(x):
                if y in full and y not in kept:
                    kept.add(y)
                    nxt.append(y)
        if not nxt:
            break
        frontier, level = nxt, level + 1
    return full, kept, level


def successors(x, kept):
    """the successor strings of the k-mer string x inside `kept`"""
    return sorted(x[1:] + c for c in ORDER if canon(x[1:] + c) in kept)


def _no_runs(rng, n, alphabet, k):
    """a sequence over two letters without a run of k - 1 equal letters"""
    out = []
    for _ in range(n):
        c = alphabet[rng.next() & 1]
        if len(out) >= 2 and out[-1] == out[-2] == c:
            c = alphabet[0] if c == alphabet[1] else alphabet[1]
        out.append(c)
    return "".join(out)


def reach_workload(k, solid, seed=5):
    """(seqs, set_lists, shared, set_shared, gaps): one gap a set (None: no gap).  The shared list is mostly unrelated
    reads (no k-mer of theirs is a neighbour of a k-mer of the genome) plus reads that extend the own windows, so a
    flagged set with a record keeps a proper, non-empty part of its full graph at every radius.  Every read is listed
    `solid` times, except in set 5, whose window is once in its own list and once in the shared list.
      0 flagged, 1 not: gaps inside their windows, the shared reads extending the window to the right;
      2 flagged, 3 not: the same reads; the tests give them no record;
      4 flagged: its gap's flanks are in no read (no seed in the graph);
      5 flagged: solid only through own + shared copies together;
      6 flagged, no own reads: the gap's flanks (set 4's window) are in a shared read;
      7 not flagged: a left flank shorter than k + lmf (the fill rejects the gap: no seeds)."""
    small = k < 11
    rng = cases.SplitMix(seed * 1000 + k)
    if small:
        genome = cases.one_strand_genome(seed + k, 260, "AC")  # dense and cyclic: 2^k possible k-mers
        other = _no_runs(rng, 200, "AT", k)
        unrelated = [_no_runs(rng, 60, "AG", k) for _ in range(5)]
        pad, gl = 6, 12
    else:
        genome = cases.random_dna(rng, 14 * k + 900)
        other = cases.random_dna(rng, 4 * k)
        unrelated = [cases.random_dna(rng, 300) for _ in range(6)]
        pad, gl = 40, 30
    lmf, rmf = 3, 2
    seqs, index = [], {}

    def entry(text):
        if text not in index:
            index[text] = len(seqs)
            seqs.append(text)
        return index[text]

    def gap_at(text, pos, lmf=lmf, rmf=rmf):
        return dict(left=text[pos - k - lmf:pos], right=text[pos + gl:pos + gl + k + rmf], gap_len=gl + k, lmf=lmf, rmf=rmf)

    def window(pos):
        return max(0, pos - k - lmf - pad), pos + gl + k + rmf + pad
    step = (len(genome) - 2 * (k + pad + 10) - gl - 4 * k) // 4
    pos = [k + lmf + pad + 5 + j * step for j in range(4)]
    ext = []
    set_lists, set_shared, gaps = [], [], []
    for j, flagged in ((0, 1), (1, 0), (0, 1), (1, 0)):   # sets 0-3
        lo, hi = window(pos[j])
        set_lists.append([entry(genome[lo:hi])] * solid)
        set_shared.append(flagged)
        gaps.append(gap_at(genome, pos[j]))
    for j in (0, 1):
        hi = window(pos[j])[1]
        ext.append(entry(genome[hi - k - 4:hi + 3 * k]))
    set_lists.append([entry(genome[window(pos[2])[0]:window(pos[2])[1]])] * solid)  # 4
    set_shared.append(1)
    gaps.append(gap_at(other, k + lmf + 2))
    lo, hi = window(pos[3])                                                          # 5
    w5 = entry(genome[lo:hi])
    set_lists.append([w5] * (solid - 1) if solid > 1 else [w5])
    set_shared.append(1)
    gaps.append(gap_at(genome, pos[3]))
    set_lists.append([])                                                             # 6
    set_shared.append(1)
    gaps.append(gap_at(genome, pos[2]))
    set_lists.append([entry(genome[window(pos[0])[0]:window(pos[0])[1]])] * solid)   # 7
    set_shared.append(0)
    bad = gap_at(genome, pos[0])
    bad["left"] = bad["left"][1:]
    gaps.append(bad)
    shared = []
    for u in unrelated:
        shared += [entry(u)] * solid
    for e in ext:
        shared += [e] * solid
    shared += [w5]  # once: only with set 5's own copies does it reach solid = 2
    shared += [entry(genome[window(pos[2])[0]:window(pos[2])[1]])] * solid  # set 6 finds its gap's flanks here
    return seqs, set_lists, shared, set_shared, gaps


NO_RECORD = (2, 3)


def reach_list(P, gaps, radius, without=NO_RECORD):
    return [None if (s in without or g is None) else (P.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"]), radius)
            for s, g in enumerate(gaps)]


def assert_matches_model(u, seqs, set_lists, shared, set_shared, gaps, radii, k, solid, outside=()):
    """every set of graph u against the model: the k-mers (count, membership of every k-mer of the full set and of
    `outside`), and every kept k-mer's successors.  radii: per set, None or the radius.  Returns [(full, kept)]."""
    from gap2seq_amd import lib as P
    assert u.num_sets == len(set_lists)
    sizes = []
    for s, own in enumerate(set_lists):
        flagged = bool(set_shared is not None and set_shared[s])
        full, kept, _ = model_set(seqs, own, shared, flagged, gaps[s], radii[s], k, solid)
        assert u.set_nodes(s)[1] == len(kept), "set %d: %d k-mers, the model keeps %d of %d" % (s, u.set_nodes(s)[1], len(kept), len(full))
        for x in list(full) + [canon(y) for y in outside]:
            v = u.set_node(s, x)
            assert (v != P.G2S_INVALID_NODE) == (x in kept), "set %d k-mer %s" % (s, x)
            if x in kept:
                assert sorted(u.node_string(w) for w in u.successors(v)) == successors(u.node_string(v), kept), (s, x)
                assert sorted(u.node_string(w) for w in u.successors(v ^ 1)) == successors(u.node_string(v ^ 1), kept), (s, x)
        sizes.append((len(full), len(kept)))
    assert u.validate() == (0, "")
    return sizes
