"""Read pools on the host: the batched read filter handing over every selected read once with per-gap index lists
(g2s_filter_reads_gaps_pool, gap2seq_amd/csrc/readfilter_gaps.cpp) and the set graph built from such a pool without
its expanded lists (g2s_graph_build_pool, gap2seq_amd/csrc/dbg.cpp).  The pool's text must be the per-gap filter's,
byte for byte; the pooled graph must be g2s_graph_build_sets' for the expanded lists, set by set.  CPU only: the host
build (G2S_HOST_BUILD=1) and the host joins (device -1); tests/test_gpu_read_pool.py runs the device paths."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import filter_gap_cases as FC  # noqa: E402
import pool_cases as PC  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402

KS = [11, 12, 31, 32, 63, 64, 95]


@pytest.fixture(autouse=True)
def _host_build(monkeypatch):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")


# ---- the filter's pool

@pytest.mark.parametrize("case", FC.all_cases(), ids=lambda c: c[0])
def test_pool_text_equals_the_batched_filter(case):
    _, bam, mean, sd, gaps = case
    want, _, un = P.filter_reads_gaps(bam, mean, sd, gaps, device=-1, unmapped=True)
    pool = P.filter_reads_gaps_pool(bam, mean, sd, gaps, device=-1)
    try:
        assert pool.stats["on_device"] == 0 and pool.stats["file_passes"] == 2
        assert pool.n_gaps == len(gaps)
        for i, g in enumerate(gaps):
            assert pool.fasta(i) == want[i][0], g
            assert len(pool.gap_reads(i)) == want[i][3]
            assert pool.total == want[i][4]
        assert pool.unmapped_fasta() == un[0] and len(pool.unmapped) == un[3] and pool.total == un[4]
        assert list(pool.unmapped) == sorted(set(pool.unmapped))
        held = set(pool.unmapped)
        for i in range(len(gaps)):
            held.update(pool.gap_reads(i))
        assert held == set(range(pool.n_reads))  # nothing held that no list names
    finally:
        pool.free()


def test_names_and_unmapped_are_optional():
    bam, _, gaps = FC.simulated(1)
    full = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1)
    bare = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1, names=False, unmapped=False)
    try:
        assert bare.names is None and list(bare.unmapped) == []
        with pytest.raises(ValueError):
            bare.fasta(0)
        for i in range(len(gaps)):  # the same reads, whatever else the pool holds
            assert [bare.seqs[r] for r in bare.gap_reads(i)] == [full.seqs[r] for r in full.gap_reads(i)]
        assert bare.n_reads <= full.n_reads and bare.nbytes < full.nbytes
    finally:
        full.free()
        bare.free()


def test_the_pool_does_not_grow_with_the_gaps():
    bam, scafs, gaps = FC.simulated(2, shuffle=True)
    gap = next(g for g in gaps if g[0] in scafs and g[3] > 0)
    pools = [P.filter_reads_gaps_pool(bam, 300, 20, [gap] * m, device=-1, unmapped=False) for m in (1, 8, 64)]
    try:
        assert len(pools[0].gap_reads(0)) > 0
        reads = pools[0].n_reads
        per_gap = 4 * len(pools[0].gap_reads(0)) + 8
        for pool, m in zip(pools, (1, 8, 64)):
            assert pool.n_reads == reads
            # (nbytes: the reads' arrays, the same whatever m is, plus every gap's index list)
            assert pool.nbytes - m * per_gap == pools[0].nbytes - per_gap
            for i in range(m):
                assert pool.gap_reads(i) == pools[0].gap_reads(0)
    finally:
        for pool in pools:
            pool.free()


def test_an_unmapped_read_a_gap_selects_is_one_entry():
    """the unmapped mate of a read in a gap's window is selected by that gap and is in the unmapped list: one pool
    entry, named by both"""
    bam, _, gaps = FC.simulated(1)
    pool = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1)
    try:
        un = set(pool.unmapped)
        both = [(i, r) for i in range(len(gaps)) for r in pool.gap_reads(i) if r in un]
        assert both, "the fixture has no unmapped read that a gap selects"
        i, r = both[0]
        record = ">" + pool.names[r].decode("latin-1") + "\n" + pool.seqs[r].decode() + "\n"
        assert record in pool.fasta(i) and record in pool.unmapped_fasta()
        assert list(pool.unmapped).count(r) == 1
    finally:
        pool.free()


def test_path_and_bytes_agree(tmp_path):
    bam, _, gaps = FC.simulated(3)
    path = tmp_path / "lib.bam"
    path.write_bytes(bam)
    a = P.filter_reads_gaps_pool(str(path), 300, 20, gaps, device=-1)
    b = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1)
    try:
        assert a.seqs == b.seqs and a.names == b.names and list(a.unmapped) == list(b.unmapped)
        assert [a.gap_reads(i) for i in range(len(gaps))] == [b.gap_reads(i) for i in range(len(gaps))]
    finally:
        a.free()
        b.free()


def test_pool_errors_leave_the_output_alone(tmp_path):
    lib = P.load_library()
    bam, _, gaps = FC.simulated(1)
    with pytest.raises(P.G2SError):
        P.filter_reads_gaps_pool(str(tmp_path / "missing.bam"), 300, 20, gaps, device=-1)
    with pytest.raises(P.G2SError):
        P.filter_reads_gaps_pool(bam[:len(bam) // 2], 300, 20, gaps, device=-1)
    out = C.POINTER(P.g2s_read_pool)()
    o = P.g2s_filter_opts(300, 20, 0, -1, -1, 0, 0, b"")
    rc = lib.g2s_filter_reads_gaps_pool(str(tmp_path / "missing.bam").encode(), C.byref(o), None, 0, -1, 1, 1, C.byref(out), None, None)
    assert rc == -2 and not out
    lib.g2s_read_pool_free(None)


# ---- the pooled set build

@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_pool_graph_equals_set_graph_of_the_expanded_lists(k, solid):
    for mode in ("shared", "empty", "none"):
        seqs, set_lists, shared, set_shared = PC.pool_workload(k, mode)
        sets = PC.expanded(seqs, set_lists, shared, set_shared)
        u = P.Graph.from_pool(seqs, set_lists, k, solid, shared=shared, set_shared=set_shared, nthreads=3)
        w = P.Graph.from_sets(sets, k, solid, nthreads=3)
        try:
            PC.assert_same_graph(u, w, len(set_lists))
            PC.assert_workload_properties(u, seqs, k, solid, mode)
            info = P.test_last_pool_build()
            own = sum(len(seqs[i]) + 1 for lst in set_lists for i in lst)
            sh = sum(len(seqs[i]) + 1 for i in shared) if set_shared and any(set_shared) else 0
            assert info == dict(own_positions=own, shared_positions=sh, keys_sorted=own + sum(set_shared or []) * sh,
                                on_device=0)
        finally:
            u.free()
            w.free()


def test_one_set_pool_is_an_ordinary_graph():
    k = 31
    seqs, _, _, _ = PC.pool_workload(k)
    u = P.Graph.from_pool(seqs, [[0, 1, 0]], k, 2, shared=[3, 3], set_shared=[1])
    g = P.Graph.from_seqs([seqs[0], seqs[1], seqs[0], seqs[3], seqs[3]], k, 2)
    try:
        assert u.num_sets == 1 and u.num_kmers == g.num_kmers > 0 and u.num_unitigs == g.num_unitigs
        for q in (seqs[0], seqs[3]):
            assert u.node(q[:k]) == g.node(q[:k]) != P.G2S_INVALID_NODE
        assert u.node(seqs[1][-k:]) == P.G2S_INVALID_NODE
    finally:
        u.free()
        g.free()


def test_pool_build_arguments():
    lib = P.load_library()
    seqs = [b"ACGTACGTTTGACCA" * 4, b"TTGACCAGGATCCAT" * 4]
    arr = (C.c_char_p * 2)(*seqs)
    lens = (C.c_uint64 * 2)(*[len(s) for s in seqs])
    u64, u32, u8 = C.c_uint64, C.c_uint32, C.c_uint8

    def build(begin, own, shared, flags, nsets, k):
        h = C.c_void_p()
        rc = lib.g2s_graph_build_pool(arr, lens, 2, (u64 * len(begin))(*begin), (u32 * max(1, len(own)))(*own),
                                      (u32 * len(shared))(*shared) if shared else None, len(shared),
                                      (u8 * len(flags))(*flags) if flags else None, nsets, k, 1, 1, C.byref(h))
        if rc != 0:
            assert h.value is None  # *out untouched
        return rc, h

    assert build([0, 1, 2], [0, 2], [], None, 2, 11)[0] == -1       # own index out of range
    assert build([0, 1, 2], [0, 1], [2], [1, 0], 2, 11)[0] == -1    # shared index out of range (flagged ...)
    assert build([0, 1, 2], [0, 1], [7], None, 2, 11)[0] == -1      # ... or not)
    assert build([0, 2, 1], [0, 1], [], None, 2, 11)[0] == -1       # set_begin decreases
    assert build([0], [], [], None, 0, 11)[0] == -1                 # no sets
    assert build([0, 1, 2], [0, 1], [], None, 2, 0)[0] == -1        # k out of range
    assert build([0, 1, 2], [0, 1], [], None, 2, 128)[0] == -1
    rc, h = build([0, 1, 2], [0, 1], [1], [0, 1], 2, 11)
    assert rc == 0 and h.value
    g = P.Graph(h)
    try:
        assert g.num_sets == 2 and g.set_node(0, seqs[1][:11].decode()) == P.G2S_INVALID_NODE
        assert g.set_node(1, seqs[1][:11].decode()) != P.G2S_INVALID_NODE
    finally:
        g.free()
