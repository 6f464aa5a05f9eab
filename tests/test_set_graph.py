"""Set graphs on the host (g2s_graph_build_sets): one graph per read set in one handle, numbered set-major, for the
wrapper's per-gap libraries flow (Gap2Seq.py:133-218).  Every set's part must be the graph g2s_graph_build_seqs gives
for that set's sequences alone — the same solid k-mers, the same successors — with no edge leaving the set.
No GPU: the set build runs on host threads, and so does the single build it is compared with."""
import ctypes as C

import pytest

import cases

KS = [21, 31, 32, 63, 64, 127]


def _sets(k):
    """overlapping windows of one genome (twice each: solid at 2), a set of one copy only, an empty set, a set of
    reads shorter than k, a set that repeats another one"""
    rng = cases.SplitMix(500 + k)
    g = cases.random_dna(rng, 1200)
    w = [g[0:400], g[250:700], g[600:1000], g[900:1200]]
    return [
        [w[0], w[0]],
        [w[1], w[1], g[100:300]],
        [w[2]],                      # each k-mer once: nothing solid at 2
        [],
        [g[:k - 1], g[5:k + 3 - 4]],  # shorter than k
        [w[3], w[3].lower(), w[1][:200]],
        [w[0], w[0]],                # the same reads as set 0: the same k-mers, other nodes
    ]


def _kmers_of(graph, first, cnt):
    return {graph.node_string(2 * i) for i in range(first, first + cnt)}


def _check_set(product, u, s, seqs, k, solid):
    first, cnt = u.set_nodes(s)
    single = product.Graph.from_seqs(seqs, k, solid, nthreads=1) if seqs else None
    try:
        assert cnt == (single.num_kmers if single else 0)
        if cnt == 0:
            for q in seqs:
                if len(q) >= k:
                    assert u.set_node(s, q[:k]) == product.G2S_INVALID_NODE
            return
        ks = _kmers_of(u, first, cnt)
        assert ks == _kmers_of(single, 0, single.num_kmers)
        lo, hi = 2 * first, 2 * (first + cnt)
        for x in ks:
            v, w = u.set_node(s, x), single.node(x)
            assert lo <= v < hi and u.node_string(v) == x
            for a, b in ((v, w), (v ^ 1, w ^ 1)):
                su, ss = u.successors(a), single.successors(b)
                assert all(lo <= t < hi for t in su)
                assert [u.node_string(t) for t in su] == [single.node_string(t) for t in ss]
                pu = u.predecessors(a)
                assert all(lo <= t < hi for t in pu)
                assert [u.node_string(t) for t in pu] == [single.node_string(t) for t in single.predecessors(b)]
    finally:
        if single:
            single.free()


@pytest.mark.parametrize("k", KS)
def test_set_graph_equals_graph_of_each_set(product, k):
    sets = _sets(k)
    for solid in (1, 2):
        u = product.Graph.from_sets(sets, k, solid, nthreads=3)
        try:
            assert u.num_sets == len(sets)
            firsts = [u.set_nodes(s) for s in range(len(sets))]
            assert firsts[0][0] == 0
            for s in range(1, len(sets)):  # set-major: the ranges follow one another in set order
                assert firsts[s][0] == firsts[s - 1][0] + firsts[s - 1][1]
            assert firsts[-1][0] + firsts[-1][1] == u.num_kmers
            for s, seqs in enumerate(sets):
                _check_set(product, u, s, seqs, k, solid)
            assert u.validate() == (0, "")
            assert u.set_nodes(3)[1] == 0 and u.set_nodes(4)[1] == 0
            if solid == 2:
                assert u.set_nodes(2)[1] == 0  # seen once in its own set
            assert u.set_nodes(6)[1] == u.set_nodes(0)[1] > 0
            x = sets[0][0][:k]
            assert u.set_node(0, x) != u.set_node(6, x)
        finally:
            u.free()


@pytest.mark.parametrize("k", [31, 64])
def test_solidity_is_counted_per_set(product, k):
    """a read seen once in each of two sets: at solid 2 none of its k-mers is solid in either set (a single graph of
    both sets' reads would keep them all)"""
    rng = cases.SplitMix(77 + k)
    a, b = cases.random_dna(rng, 300), cases.random_dna(rng, 300)
    u = product.Graph.from_sets([[a, b, b], [a]], k, 2)
    both = product.Graph.from_seqs([a, a], k, 2)
    try:
        assert both.num_kmers > 0 and both.node(a[:k]) != product.G2S_INVALID_NODE
        first, cnt = u.set_nodes(0)
        assert cnt == len({pyref_canon(b[i:i + k]) for i in range(len(b) - k + 1)})
        assert u.set_nodes(1) == (cnt, 0)
        assert u.set_node(0, a[:k]) == product.G2S_INVALID_NODE
        assert u.set_node(1, a[:k]) == product.G2S_INVALID_NODE
        assert u.set_node(0, b[:k]) != product.G2S_INVALID_NODE
        assert u.validate()[0] == 0
    finally:
        u.free()
        both.free()


def pyref_canon(x):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rc = "".join(comp[c] for c in reversed(x))
    # GATB codec order A0 C1 T2 G3
    key = {"A": "0", "C": "1", "T": "2", "G": "3"}
    return min(x, rc, key=lambda s: "".join(key[c] for c in s))


@pytest.mark.parametrize("k", [31, 32, 127])
def test_one_set_graph_is_an_ordinary_graph(product, k):
    rng = cases.SplitMix(31337 + k)
    seqs = [cases.random_dna(rng, 500) for _ in range(3)]
    seqs.append(seqs[0][100:400])
    u = product.Graph.from_sets([seqs], k, 2, nthreads=2)
    g = product.Graph.from_seqs(seqs, k, 2, nthreads=2)
    try:
        assert u.num_sets == g.num_sets == 1
        assert u.set_nodes(0) == (0, g.num_kmers) and u.num_kmers == g.num_kmers > 0
        assert u.num_unitigs == g.num_unitigs
        for i in range(len(seqs[0]) - k + 1):
            x = seqs[0][i:i + k]
            assert u.node(x) == g.node(x) == u.set_node(0, x)
        assert u.validate()[0] == 0
    finally:
        u.free()
        g.free()


def test_set_graph_arguments(product, tmp_path):
    lib = product.load_library()
    seqs = [b"ACGTACGTTTGACCA" * 4, b"TTGACCAGGATCCAT" * 4]
    arr = (C.c_char_p * 2)(*seqs)
    lens = (C.c_uint64 * 2)(*[len(s) for s in seqs])
    h = C.c_void_p()
    assert lib.g2s_graph_build_sets(arr, lens, (C.c_uint32 * 2)(0, 2), 2, 2, 11, 1, 1, C.byref(h)) == -1  # set id >= nsets
    assert lib.g2s_graph_build_sets(arr, lens, (C.c_uint32 * 2)(0, 0), 2, 0, 11, 1, 1, C.byref(h)) == -1  # no sets
    assert lib.g2s_graph_build_sets(arr, lens, (C.c_uint32 * 2)(1, 0), 2, 2, 0, 1, 1, C.byref(h)) == -1   # k out of range
    u = product.Graph.from_sets([[s.decode()] for s in seqs], 11, 1)
    try:
        assert u.num_sets == 2
        x = seqs[0][:11].decode()
        assert u.set_node(0, x) != product.G2S_INVALID_NODE
        assert u.node(x) == product.G2S_INVALID_NODE  # several sets: the set must be named
        assert u.set_node(2, x) == product.G2S_INVALID_NODE
        with pytest.raises(product.G2SError) as e:
            u.set_nodes(2)
        assert e.value.code == -1
        with pytest.raises(product.G2SError) as e:
            u.save(str(tmp_path / "sets.g2s"))
        assert e.value.code == -1
    finally:
        u.free()
