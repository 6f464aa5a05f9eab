"""Designed reads for graph builds at even k, shared by tests/test_even_k_host.py (host build) and
tests/test_gpu_even_k_build.py (device build).

At even k a k-mer can be its own reverse complement (a palindrome).  The host build (gap2seq_amd/csrc/dbg.cpp:
build_tables_rank, unitig_order, build_ustart) is the authority on what happens then:
  * only strand 1 of a palindrome exists; a neighbour that is a palindrome is named with orientation 1;
  * predecessors come from an explicit table (pred(v) = succ(v ^ 1) ^ 1 does not hold next to a palindrome);
  * an edge v -> w is unitig-internal only if the one out-edge of w ^ 1 leads back to v ^ 1;
  * a k-mer's numbering walk starts on strand 1 when its strand-0 row is empty and strand 1 has an out-edge.
The reads below meet each rule at least once at every even k; `designed` names the palindromes they were built around,
and the tests assert on the host graph that those are there."""
import cases
import pyref


def palindrome(rng, k):
    half = cases.random_dna(rng, k // 2)
    return half + pyref.revcomp(half)


def _not_mirrored(a, b):
    """b with a first base that is not the complement of a's last: a + palindrome + b then gives the palindrome two
    successors (b's first base, and the reverse strand of the k-mer in front of it)"""
    if b[0] != pyref.revcomp(a[-1]):
        return b
    return "ACGT"[("ACGT".index(b[0]) + 1) & 3] + b[1:]


def designed_reads(k, solid):
    """(reads, designed): every read `solid` times; designed = dict(name -> palindromic k-mer)"""
    assert k % 2 == 0
    rng = cases.SplitMix(7000 + k)
    pad = k + 9
    reads, designed = [], {}
    # a hairpin: the k-mer at its centre is a palindrome whose only successor is its predecessor's reverse strand
    s = cases.random_dna(rng, pad)
    reads.append(s + pyref.revcomp(s))
    designed["hairpin"] = s[len(s) - k // 2:] + pyref.revcomp(s)[:k // 2]
    # period 4 and period 2: a palindrome's successor is a palindrome, k-mers that follow themselves or their own
    # reverse strand
    for unit in ("ACGT", "AT"):
        r = unit * ((k + 8) // len(unit) + 1)
        reads.append(r)
        pals = [r[i:i + k] for i in range(len(r) - k + 1) if r[i:i + k] == pyref.revcomp(r[i:i + k])]
        designed["period%d" % len(unit)] = pals[0]
    # a palindrome in the middle of an otherwise non-branching path, and one that ends a path: out-degree 1, and the
    # edge back from its successor's other strand leads to the palindrome itself, not to its (empty) strand 0
    a, b, p = cases.random_dna(rng, pad), cases.random_dna(rng, pad), palindrome(rng, k)
    reads.append(a + p + _not_mirrored(a, b))
    designed["middle"] = p
    a, p = cases.random_dna(rng, pad), palindrome(rng, k)
    reads.append(a + p)
    designed["end"] = p
    # a palindrome next to a branch: a second read leaves the path one base before the palindrome, a third joins it
    # one base behind it
    a, b, p = cases.random_dna(rng, pad), cases.random_dna(rng, pad), palindrome(rng, k)
    path = a + p + _not_mirrored(a, b)
    at = len(a) + k - 1  # the palindrome's last base
    other = "ACGT"[("ACGT".index(path[at]) + 1) & 3]
    reads.append(path)
    reads.append(path[:at] + other + cases.random_dna(rng, pad))
    reads.append(cases.random_dna(rng, pad) + "ACGT"[("ACGT".index(path[len(a)]) + 2) & 3] + path[len(a) + 1:])
    designed["branch"] = p
    # an isolated palindrome: no edge at all
    p = palindrome(rng, k)
    reads.append(p)
    designed["isolated"] = p
    # tandem reads: a cycle through a palindrome, and a circular unitig without one
    p = palindrome(rng, k)
    reads.append((p + cases.random_dna(rng, 17)) * 4)
    designed["tandem"] = p
    reads.append(cases.random_dna(rng, k + 21) * 4)
    # random reads around them: coverage 3 of a random genome, one read with an N
    genome = cases.random_dna(rng, 900 + 6 * k)
    rl = 2 * k + 60
    for i in range(0, len(genome) - rl, rl // 3):
        reads.append(genome[i:i + rl])
    reads.append(genome[40:40 + rl][:k + 5] + "N" + genome[40:40 + rl][k + 6:])
    reads.append(genome[:k - 1])
    return [r for r in reads for _ in range(solid)], designed


def graph_map(g):
    """every oriented node: string -> (successor strings, predecessor strings), GATB order (the method of
    tests/test_gpu_kmer_widths.py: _graph_map)"""
    out = {}
    for v in range(2 * g.num_kmers):
        s = g.node_string(v)
        w = g.node(s)
        if s == pyref.revcomp(s):  # a palindrome: both ids spell it; the one node() gives carries the edges
            assert w in (v, v ^ 1), (v, s)
        else:
            assert w == v and s not in out, (v, s)
        if w == v:
            out[s] = (tuple(g.node_string(x) for x in g.successors(v)), tuple(g.node_string(x) for x in g.predecessors(v)))
        else:  # the palindrome's other id: strand 0, which does not exist
            assert g.successors(v) == [] and g.predecessors(v) == [], (v, s)
    return out


def assert_graph_is_pyrefs(g, reads, k, solid, designed):
    """graph g against pyref.Graph by node string, successors and predecessors of every oriented node; the designed
    palindromes are nodes of it.  Returns the map."""
    m = graph_map(g)
    p = pyref.Graph(reads, k, solid)
    assert {pyref.canon(s)[0] for s in m} == p.kmers
    for s, (succ, pred) in m.items():
        assert list(succ) == p.succ(s) and list(pred) == p.pred(s), s
    assert g.validate() == (0, "")
    for name, pal in designed.items():
        assert pal == pyref.revcomp(pal) and len(pal) == k, name
        assert pal in m, "the %s palindrome is not in the graph" % name
    if k >= 12:  # (below, the random reads hold most k-mers there are and the designed neighbourhoods merge)
        assert m[designed["isolated"]] == ((), ())
        assert len(m[designed["hairpin"]][0]) == 1 and len(m[designed["end"]][0]) == 1
        assert len(m[designed["middle"]][0]) == 2 and len(m[designed["branch"]][0]) >= 2
        nxt = m[designed["period2"]][0]
        assert len(nxt) == 1 and nxt[0] == pyref.revcomp(nxt[0]) and nxt[0] != designed["period2"]
    return m
