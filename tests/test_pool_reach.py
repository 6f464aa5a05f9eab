"""Pooled set graphs bounded by reach records on the host (g2s_graph_build_pool_reach, gap2seq_amd/csrc/dbg.cpp:
build_pool_reach_host): every set with a record against a brute-force model of the definition in include/g2s.h
(tests/reach_cases.py), k-mer by k-mer; the build without records against g2s_graph_build_pool; the argument errors;
the test hook.  CPU only (G2S_HOST_BUILD=1); tests/test_gpu_pool_reach.py runs the device search against this path."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import cases  # noqa: E402
import pool_cases as PC  # noqa: E402
import reach_cases as RC  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402

KS = [5, 7, 31, 32, 63, 64, 95]
ERR_ARG = -1  # G2S_ERR_ARG (include/g2s.h)


@pytest.fixture(autouse=True)
def _host_build(monkeypatch):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")


def _diameter(seqs, set_lists, shared, set_shared, gaps, k, solid):
    """the deepest level any set's unbounded search reaches: at this radius every set keeps its seeds' whole component"""
    return max(RC.model_set(seqs, own, shared, bool(set_shared[s]), gaps[s], 10 ** 9, k, solid)[2]
               for s, own in enumerate(set_lists) if s not in RC.NO_RECORD)


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_reach_sets_equal_the_model(k, solid):
    seqs, set_lists, shared, set_shared, gaps = RC.reach_workload(k, solid)
    diam = _diameter(seqs, set_lists, shared, set_shared, gaps, k, solid)
    assert diam > 12 or k < 11
    rng = cases.SplitMix(k)
    outside = [cases.random_dna(rng, k) for _ in range(20)] + [g["left"][:k] for g in gaps]
    for radius in (0, 1, 12, diam, -1):
        u = P.Graph.from_pool(seqs, set_lists, k, solid, shared=shared, set_shared=set_shared,
                              reach=RC.reach_list(P, gaps, radius))
        info = P.test_last_pool_reach()
        try:
            radii = [None if s in RC.NO_RECORD else radius for s in range(len(set_lists))]
            sizes = RC.assert_matches_model(u, seqs, set_lists, shared, set_shared, gaps, radii, k, solid, outside)
        finally:
            u.free()
        if radius < 0:   # every set whole: no record at all
            assert all(f == kp for f, kp in sizes)
            continue
        with_record = [s for s in range(len(set_lists)) if s not in RC.NO_RECORD]
        assert info["reach_sets"] == len(with_record) and info["on_device"] == 0
        assert info["full_kmers"] == sum(sizes[s][0] for s in with_record)
        assert info["kept_kmers"] == sum(sizes[s][1] for s in with_record)
        assert info["levels"] <= radius and (info["levels"] == radius or radius > 1)
        # the cases the workload exists for
        for s in (0, 5, 6):                       # flagged, a seed in the graph: a proper part, never nothing
            assert 0 < sizes[s][1] < sizes[s][0], (s, radius, sizes[s])
        assert sizes[1][1] > 0 and sizes[4] == (sizes[4][0], 0) and sizes[7] == (sizes[7][0], 0) and sizes[4][0] > 0
        assert sizes[2][1] == sizes[2][0] > 0 and sizes[3][1] == sizes[3][0] > 0  # no record
        if radius == 0:
            assert sizes[0][1] <= (3 + 1) + 2 * (2 + 1)
        if radius == diam and k >= 11:
            assert sizes[1][1] == sizes[1][0]     # not flagged: its window is one component
    if solid == 2 and k >= 11:  # (at k = 5 and 7 every k-mer is everywhere) set 5's seeds are solid through its own copy and the shared copy together, through neither alone
        seed = RC.seeds_of(gaps[5], k)[0]
        own = RC.kmer_counts([seqs[i] for i in set_lists[5]], k)
        sh = RC.kmer_counts([seqs[i] for i in shared], k)
        assert own[seed] == 1 and sh[seed] == 1


@pytest.mark.parametrize("k", [31, 32, 95])
def test_without_records_the_graph_is_the_pool_builds(k):
    for mode in ("shared", "empty", "none"):
        seqs, set_lists, shared, set_shared = PC.pool_workload(k, mode)
        want = P.Graph.from_pool(seqs, set_lists, k, 2, shared=shared, set_shared=set_shared)
        blank = P.Gap("ACGT" * 40, "ACGT" * 40, 10, 2, 2)
        got = P.Graph.from_pool(seqs, set_lists, k, 2, shared=shared, set_shared=set_shared,
                                reach=[(blank, -1) if s % 2 else None for s in range(len(set_lists))])
        try:
            PC.assert_same_graph(got, want, len(set_lists))
        finally:
            got.free()
            want.free()


def _raw_args(seqs, begin, own, shared, flags):
    enc = [s.encode() for s in seqs]
    u64, u32, u8 = C.c_uint64, C.c_uint32, C.c_uint8
    return ((C.c_char_p * len(enc))(*enc), (u64 * len(enc))(*[len(e) for e in enc]), len(enc), (u64 * len(begin))(*begin),
            (u32 * max(1, len(own)))(*own), (u32 * max(1, len(shared)))(*shared), len(shared), (u8 * len(flags))(*flags),
            len(flags))


def test_null_arrays_and_argument_errors():
    lib = P.load_library()
    k = 31
    seqs, set_lists, shared, set_shared = PC.pool_workload(k, "shared")
    begin, own = [0], []
    for lst in set_lists:
        own += lst
        begin.append(len(own))
    args = _raw_args(seqs, begin, own, shared, set_shared)
    n = len(set_lists)
    gaps, keep = P._gap_array([P.Gap(seqs[0][:k + 2], seqs[1][:k + 2], 20, 2, 2)] * n)
    radius = (C.c_int32 * n)(*([5] * n))
    # both arrays NULL: g2s_graph_build_pool's graph
    h = C.c_void_p()
    assert lib.g2s_graph_build_pool_reach(*args, k, 1, 0, None, None, C.byref(h)) == P.G2S_OK
    got, want = P.Graph(h), P.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared)
    try:
        PC.assert_same_graph(got, want, n)
    finally:
        got.free()
        want.free()
    # one of the two NULL, and g2s_graph_build_pool's own errors
    h = C.c_void_p()
    assert lib.g2s_graph_build_pool_reach(*args, k, 1, 0, gaps, None, C.byref(h)) == ERR_ARG and not h
    assert lib.g2s_graph_build_pool_reach(*args, k, 1, 0, None, radius, C.byref(h)) == ERR_ARG and not h
    assert lib.g2s_graph_build_pool_reach(*args, 0, 1, 0, gaps, radius, C.byref(h)) == ERR_ARG and not h
    assert lib.g2s_graph_build_pool_reach(*args, 128, 1, 0, gaps, radius, C.byref(h)) == ERR_ARG and not h
    assert lib.g2s_graph_build_pool_reach(*args[:8], 0, k, 1, 0, gaps, radius, C.byref(h)) == ERR_ARG and not h
    bad = _raw_args(seqs, begin, [len(seqs)] + own[1:], shared, set_shared)
    assert lib.g2s_graph_build_pool_reach(*bad, k, 1, 0, gaps, radius, C.byref(h)) == ERR_ARG and not h
    bad = _raw_args(seqs, begin, own, [len(seqs)], set_shared)
    assert lib.g2s_graph_build_pool_reach(*bad, k, 1, 0, gaps, radius, C.byref(h)) == ERR_ARG and not h
    bad = _raw_args(seqs, [0, 3, 2] + begin[3:], own, shared, set_shared)
    assert lib.g2s_graph_build_pool_reach(*bad, k, 1, 0, gaps, radius, C.byref(h)) == ERR_ARG and not h
    with pytest.raises(ValueError):
        P.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared, reach=[None])
    del keep


@pytest.mark.parametrize("k", [31, 64])
def test_one_set_with_a_record_is_an_ordinary_graph(k):
    seqs, set_lists, shared, set_shared, gaps = RC.reach_workload(k, 1)
    g = gaps[0]
    u = P.Graph.from_pool(seqs, [set_lists[0]], k, 1, shared=shared, set_shared=[1],
                          reach=[(P.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"]), 12)])
    try:
        full, kept, _ = RC.model_set(seqs, set_lists[0], shared, True, g, 12, k, 1)
        assert u.num_sets == 1 and u.num_kmers == len(kept) and 0 < len(kept) < len(full)
        for x in full:
            assert (u.node(x) != P.G2S_INVALID_NODE) == (x in kept)
        assert u.validate() == (0, "")
    finally:
        u.free()


def test_the_sound_radius():
    g = P.Gap("A" * 40, "C" * 40, 100, 7, 5)
    assert P.reach_radius(g, 500) == 612
    assert P.reach_radius(P.Gap("A" * 40, "C" * 40, 10, 7, 5), -50) == 12
