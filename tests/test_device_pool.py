"""Device-held read pools without a device (g2s_filter_reads_gaps_dpool with device -1, g2s_graph_build_dpool_reach on the
host build): a host-held handle is the host pool of the same call, array for array and read for read; the pooled build
over two such handles gives the graph of g2s_graph_build_pool[_reach] on the same sequences; the argument errors; pools
freed before the graph is used.  tests/test_gpu_device_pool.py runs the device-held kind."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dpool_cases as DC  # noqa: E402
import pool_cases as PC  # noqa: E402


@pytest.fixture
def P(product, monkeypatch):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    return product


def _pools(P, padded, cut):
    """two host-held handles over padded[:cut] and padded[cut:]"""
    out = []
    for part in (padded[:cut], padded[cut:]):
        dp = P.filter_reads_gaps_dpool(DC.pool_bam(part), 300, 20, [], device=-1)
        assert dp.device == -1 and dp.device_bytes == 0 and dp.n_reads == len(part)
        out.append(dp)
    return out


def test_a_host_held_handle_is_the_host_pool(product):
    P = product
    bam, gaps = DC.designed_library()
    pool = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1, names=True, unmapped=True)
    dp = P.filter_reads_gaps_dpool(bam, 300, 20, gaps, device=-1)
    try:
        DC.assert_designed_properties(pool, len(gaps))
        assert dp.device == -1 and dp.device_bytes == 0
        assert dp.stats["file_passes"] == pool.stats["file_passes"] == 2
        DC.assert_same_pool(dp, pool, len(gaps))
        hook = P.test_last_dpool()
        assert hook["held_on_device"] == 0 and hook["bases_bytes_to_host"] == sum(len(s) for s in pool.seqs) > 0
        for i in range(len(gaps)):
            assert dp.gap_reads(i) == list(pool.gap_reads(i))
    finally:
        dp.free()
        pool.free()
    # without the unmapped reads
    pool = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1, names=True, unmapped=False)
    dp = P.filter_reads_gaps_dpool(bam, 300, 20, gaps, device=-1, unmapped=False)
    try:
        assert len(dp.unmapped_read) == 0
        DC.assert_same_pool(dp, pool, len(gaps))
    finally:
        dp.free()
        pool.free()


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", DC.KS)
def test_build_over_two_host_held_pools_equals_the_pool_build(P, k, solid):
    for mode in ("shared", "empty", "none"):
        padded, set_lists, shared, set_shared, cut = DC.split_workload(k, mode)
        pools = _pools(P, padded, cut)
        try:
            assert [pools[0].read(r).decode() for r in range(cut)] == padded[:cut]
            for reach in (None, DC.reach_for(P, padded, set_lists, k)):
                got = P.Graph.from_dpools(pools, set_lists, k, solid, shared=shared, set_shared=set_shared, reach=reach)
                hook = P.test_last_dpool()
                want = P.Graph.from_pool(padded, set_lists, k, solid, shared=shared, set_shared=set_shared, reach=reach)
                try:
                    PC.assert_same_graph(got, want, len(set_lists))
                    if reach is None:
                        PC.assert_workload_properties(got, PC.pool_workload(k, mode)[0], k, solid, mode)
                    else:
                        assert any(got.set_nodes(s)[1] for s, r in enumerate(reach) if r is not None)
                    in_use = {i for lst in set_lists for i in lst} | (set(shared) if set_shared and any(set_shared) else set())
                    assert hook["text_bytes_gathered_on_device"] == 0
                    assert hook["text_bytes_packed_on_host"] == sum(len(padded[i]) + 1 for i in in_use)
                finally:
                    got.free()
                    want.free()
        finally:
            for dp in pools:
                dp.free()


def test_one_set_is_an_ordinary_graph(P):
    k = 31
    padded, set_lists, shared, set_shared, cut = DC.split_workload(k, "shared")
    pools = _pools(P, padded, cut)
    try:
        for reach in (None, DC.reach_for(P, padded, set_lists[1:2], k)):
            got = P.Graph.from_dpools(pools, set_lists[1:2], k, 1, shared=shared, set_shared=[1], reach=reach)
            want = P.Graph.from_pool(padded, set_lists[1:2], k, 1, shared=shared, set_shared=[1], reach=reach)
            try:
                assert got.num_sets == want.num_sets == 1 and got.num_kmers == want.num_kmers > 0
                assert got.num_unitigs == want.num_unitigs and got.validate() == (0, "")
                assert PC.set_view(got, 0) == PC.set_view(want, 0)
            finally:
                got.free()
                want.free()
    finally:
        for dp in pools:
            dp.free()


def test_argument_errors(P):
    lib = P.load_library()
    k = 31
    padded, set_lists, shared, set_shared, cut = DC.split_workload(k, "shared")
    pools = _pools(P, padded, cut)
    try:
        hs = (C.c_void_p * 2)(*[p.h for p in pools])
        total = len(padded)
        begin = (C.c_uint64 * 3)(0, 2, 3)
        good = (C.c_uint32 * 3)(1, total - 1, 3)
        sh = (C.c_uint32 * 1)(5)
        flags = (C.c_uint8 * 2)(1, 0)
        gaps, keep = P._gap_array([P.Gap("A" * 40, "C" * 40, 10, 5, 5)] * 2)
        radius = (C.c_int32 * 2)(50, -1)
        h = C.c_void_p()

        def build(hs=hs, npools=2, seq=good, shared_seq=sh, nsets=2, g=gaps, r=radius):
            return lib.g2s_graph_build_dpool_reach(hs, npools, begin, seq, shared_seq, 1, flags, nsets, k, 1, 0, g, r, C.byref(h))
        assert build() == P.G2S_OK and h
        lib.g2s_graph_free(h)
        h = C.c_void_p()
        assert build(g=None, r=None) == P.G2S_OK and h
        lib.g2s_graph_free(h)
        h = C.c_void_p()
        assert build(seq=(C.c_uint32 * 3)(1, total, 3)) == DC.G2S_ERR_ARG and not h         # an index >= the pools' total
        assert build(seq=(C.c_uint32 * 3)(1, total, 3), g=None, r=None) == DC.G2S_ERR_ARG and not h
        assert build(shared_seq=(C.c_uint32 * 1)(total)) == DC.G2S_ERR_ARG and not h
        assert build(npools=0) == DC.G2S_ERR_ARG and not h                                  # no pools, sets asked for
        assert build(hs=None, npools=0) == DC.G2S_ERR_ARG and not h
        assert build(g=None) == DC.G2S_ERR_ARG and not h                                    # exactly one reach array
        assert build(r=None) == DC.G2S_ERR_ARG and not h
        assert build(nsets=0) == DC.G2S_ERR_ARG and not h
        assert "g2s_graph_build_dpool_reach" in lib.g2s_last_error().decode()
        del keep
        with pytest.raises(IndexError):
            pools[0].read(pools[0].n_reads)
        assert lib.g2s_device_pool_read(pools[0].h, pools[0].n_reads, None) == DC.G2S_ERR_ARG
    finally:
        for dp in pools:
            dp.free()


def test_pools_may_be_freed_before_the_graph_is_used(P):
    k = 31
    padded, set_lists, shared, set_shared, cut = DC.split_workload(k, "shared")
    pools = _pools(P, padded, cut)
    got = P.Graph.from_dpools(pools, set_lists, k, 1, shared=shared, set_shared=set_shared)
    for dp in pools:
        dp.free()
        dp.free()   # (a second free of the wrapper is nothing)
    want = P.Graph.from_pool(padded, set_lists, k, 1, shared=shared, set_shared=set_shared)
    try:
        assert got.validate() == (0, "")
        PC.assert_same_graph(got, want, len(set_lists))
    finally:
        got.free()
        want.free()
