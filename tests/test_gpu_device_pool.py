"""Device-held read pools on the MI355X: the batched read filter leaving its reads in device memory on both one-pass
routes (gap2seq_amd/csrc/bam_text.hip: pass B writes the pooled build's text) against the host pool of the same call; the
pooled build gathering its text from such pools (gap2seq_amd/csrc/dbg_gpu.hip: k_gather_reads) against the build from
host pointers and the device set build of the expanded lists; the separator between adjacent reads; pools of both kinds
in one build; fills on the graph; and Gap2Seq-libraries -device-pool against the host round trip."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import cases  # noqa: E402
import dpool_cases as DC  # noqa: E402
import filter_gap_cases as FC  # noqa: E402
import pool_cases as PC  # noqa: E402
from test_gpu_read_pool import DERR, EXE, FUZ, K, LSEED, SOLID, _fields, _fill, _gap, libraries_case  # noqa: E402

pytestmark = pytest.mark.gpu

ON_DEVICE, NOT_ASKED = 0, 1
SWITCHES = ("G2S_HOST_FILTER", "G2S_HOST_INFLATE", "G2S_DEVICE_INFLATE", "G2S_HOST_ROWS", "G2S_DEVICE_ROWS", "G2S_FILTER_ONE_PASS",
            "G2S_FILTER_RESIDENT_CAP", "G2S_FILTER_STORE", "G2S_FILTER_STORE_SAMPLE", "G2S_BAM_CHUNK", "G2S_HOST_BUILD",
            "G2S_DEVICE", "G2S_DEVICE_POOL")


@pytest.fixture
def P(product, monkeypatch):
    """the product with no switch set and the mode following the environment, before and after"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    product.filter_set_one_pass(-1)
    yield product
    product.filter_set_one_pass(-1)


def _held(P, bam, gaps=(), unmapped=True):
    """a device-held handle, or the test fails: never the host in the kernels' place"""
    dp = P.filter_reads_gaps_dpool(bam, 300, 20, list(gaps), device=0, unmapped=unmapped)
    text, hook = P.last_filter_text(), P.test_last_dpool()
    assert (dp.stats["file_passes"], text["one_pass"], text["reason"]) == (1, 1, ON_DEVICE), (dp.stats, text)
    assert (hook["held_on_device"], hook["bases_bytes_to_host"]) == (1, 0), hook
    assert dp.device == 0 and dp.device_bytes >= int(dp.base_off[-1]) + dp.n_reads + 8 * (dp.n_reads + 1)
    return dp


# ---- 1. the filter on each route

def _libraries():
    bam, gaps = DC.designed_library()
    big, _, big_gaps = FC.simulated(1, pairs=700)
    return [("designed", bam, gaps), ("simulated", big, big_gaps)]


@pytest.mark.parametrize("route", ["resident", "store", "forbidden"])
def test_the_handle_on_each_route_is_the_host_pool(P, monkeypatch, route):
    for label, bam, gaps in _libraries():
        P.filter_set_one_pass(0)
        pool = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1, names=True, unmapped=True)
        P.filter_set_one_pass(-1)
        if route == "store":
            monkeypatch.setenv("G2S_FILTER_STORE", "1")
        if route == "forbidden":
            P.filter_set_one_pass(0)
            dp = P.filter_reads_gaps_dpool(bam, 300, 20, gaps, device=0)
            text, hook = P.last_filter_text(), P.test_last_dpool()
            assert (dp.stats["file_passes"], text["one_pass"], text["reason"]) == (2, 0, NOT_ASKED)
            assert dp.device == -1 and dp.device_bytes == 0 and hook["held_on_device"] == 0
            assert hook["bases_bytes_to_host"] == sum(len(s) for s in pool.seqs)
        else:
            dp = _held(P, bam, gaps)
            assert P.last_filter_store()["used"] == (1 if route == "store" else 0)
        try:
            if label == "designed":
                DC.assert_designed_properties(pool, len(gaps))
            else:
                assert pool.total > 4000 and pool.n_reads > 200
            assert dp.stats["on_device"] == 1
            DC.assert_same_pool(dp, pool, len(gaps))
        finally:
            dp.free()
            pool.free()


def test_the_environment_forbids_too(P, monkeypatch):
    bam, gaps = DC.designed_library()
    monkeypatch.setenv("G2S_FILTER_ONE_PASS", "0")
    dp = P.filter_reads_gaps_dpool(bam, 300, 20, gaps[:4], device=0)
    assert dp.device == -1 and dp.stats["file_passes"] == 2
    dp.free()
    monkeypatch.setenv("G2S_FILTER_ONE_PASS", "1")
    _held(P, bam, gaps[:4]).free()


# ---- 2. the build

def _device_build(P, pools, set_lists, k, solid, **kw):
    u = P.Graph.from_dpools(pools, set_lists, k, solid, **kw)
    assert P.test_last_pool_build()["on_device"] == 1
    return u, P.test_last_dpool()


def _in_use_positions(padded, set_lists, shared, set_shared):
    in_use = {i for lst in set_lists for i in lst} | (set(shared) if set_shared and any(set_shared) else set())
    return sum(len(padded[i]) + 1 for i in in_use)


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", DC.KS)
def test_build_from_device_held_pools_equals_the_pool_build(P, k, solid):
    for mode in ("shared", "empty", "none"):
        padded, set_lists, shared, set_shared, cut = DC.split_workload(k, mode)
        pools = [_held(P, DC.pool_bam(padded[:cut])), _held(P, DC.pool_bam(padded[cut:]))]
        sets = P.Graph.from_sets(PC.expanded(padded, set_lists, shared, set_shared), k, solid) if k % 2 else None
        try:
            assert [pools[1].read(r).decode() for r in range(len(padded) - cut)] == padded[cut:]
            for reach in (None, DC.reach_for(P, padded, set_lists, k)):
                got, hook = _device_build(P, pools, set_lists, k, solid, shared=shared, set_shared=set_shared, reach=reach)
                want = P.Graph.from_pool(padded, set_lists, k, solid, shared=shared, set_shared=set_shared, reach=reach)
                try:
                    assert P.test_last_dpool()["text_bytes_gathered_on_device"] == 0   # (the build from host pointers)
                    assert hook["text_bytes_packed_on_host"] == 0
                    assert hook["text_bytes_gathered_on_device"] == _in_use_positions(padded, set_lists, shared, set_shared)
                    PC.assert_same_graph(got, want, len(set_lists))
                    if reach is None:
                        if sets is not None:
                            PC.assert_same_graph(got, sets, len(set_lists))
                        PC.assert_workload_properties(got, PC.pool_workload(k, mode)[0], k, solid, mode)
                finally:
                    got.free()
                    want.free()
        finally:
            if sets is not None:
                sets.free()
            for dp in pools:
                dp.free()


@pytest.mark.parametrize("k", [31, 30])
def test_one_set_from_device_held_pools(P, k):
    padded, set_lists, shared, set_shared, cut = DC.split_workload(k, "shared")
    pools = [_held(P, DC.pool_bam(padded[:cut])), _held(P, DC.pool_bam(padded[cut:]))]
    try:
        for reach in (DC.reach_for(P, padded, set_lists[1:2], k), None):
            got = P.Graph.from_dpools(pools, set_lists[1:2], k, 1, shared=shared, set_shared=[1], reach=reach)
            hook = P.test_last_dpool()
            want = P.Graph.from_pool(padded, set_lists[1:2], k, 1, shared=shared, set_shared=[1], reach=reach)
            try:
                if reach is not None:   # (built as two sets on the device; without records it is an ordinary graph build)
                    assert hook["text_bytes_packed_on_host"] == 0
                    assert hook["text_bytes_gathered_on_device"] == _in_use_positions(padded, set_lists[1:2], shared, [1])
                assert got.num_sets == want.num_sets == 1 and got.num_kmers == want.num_kmers > 0
                assert got.num_unitigs == want.num_unitigs and got.validate() == (0, "")
                assert PC.set_view(got, 0) == PC.set_view(want, 0)
            finally:
                got.free()
                want.free()
    finally:
        for dp in pools:
            dp.free()


# ---- 3. the separator

@pytest.mark.parametrize("k", [31, 63, 95, 30])
def test_no_kmer_spans_two_adjacent_reads(P, k):
    rng = cases.SplitMix(5 + k)
    a, b, c = (cases.random_dna(rng, n) for n in (k + 22, k + 9, 2 * k))
    dp = _held(P, DC.pool_bam([a, b, c]))
    try:
        u, hook = _device_build(P, [dp], [[0, 1], [2]], k, 1)
        try:
            absent = P.G2S_INVALID_NODE
            assert hook["text_bytes_gathered_on_device"] == len(a) + len(b) + len(c) + 3
            for cut in range(1, k):   # every k-mer over the A|B boundary
                assert u.set_node(0, (a + b)[len(a) - cut:len(a) - cut + k]) == absent, cut
            assert u.set_node(0, a[-k:]) != absent and u.set_node(0, b[:k]) != absent
            assert u.set_node(0, a[:k]) != absent and u.set_node(0, b[-k:]) != absent
            assert u.set_nodes(0)[1] == len(a) + len(b) - 2 * (k - 1)
            assert u.set_node(1, c[:k]) != absent and u.set_node(0, c[:k]) == absent
        finally:
            u.free()
    finally:
        dp.free()


# ---- 4. pools of both kinds in one build

@pytest.mark.parametrize("k", [31, 63])
def test_device_held_and_host_held_pools_in_one_build(P, monkeypatch, k):
    padded, set_lists, shared, set_shared, cut = DC.split_workload(k, "shared")
    c1, c2 = cut // 2, cut
    first = _held(P, DC.pool_bam(padded[:c1]))
    P.filter_set_one_pass(0)
    second = P.filter_reads_gaps_dpool(DC.pool_bam(padded[c1:c2]), 300, 20, [], device=0)
    P.filter_set_one_pass(-1)
    third = _held(P, DC.pool_bam(padded[c2:]))
    pools = [first, second, third]
    assert [p.device for p in pools] == [0, -1, 0]
    want = P.Graph.from_pool(padded, set_lists, k, 1, shared=shared, set_shared=set_shared)
    try:
        got, hook = _device_build(P, pools, set_lists, k, 1, shared=shared, set_shared=set_shared)
        try:
            assert hook["text_bytes_gathered_on_device"] > 0 and hook["text_bytes_packed_on_host"] > 0
            assert hook["text_bytes_gathered_on_device"] + hook["text_bytes_packed_on_host"] == \
                _in_use_positions(padded, set_lists, shared, set_shared)
            PC.assert_same_graph(got, want, len(set_lists))
        finally:
            got.free()
        # the same pools read by the host build: the device-held ones come down once
        monkeypatch.setenv("G2S_HOST_BUILD", "1")
        got = P.Graph.from_dpools(pools, set_lists, k, 1, shared=shared, set_shared=set_shared)
        hook = P.test_last_dpool()
        monkeypatch.delenv("G2S_HOST_BUILD")
        try:
            assert P.test_last_pool_build()["on_device"] == 0 and hook["text_bytes_gathered_on_device"] == 0
            assert hook["text_bytes_packed_on_host"] == _in_use_positions(padded, set_lists, shared, set_shared)
            PC.assert_same_graph(got, want, len(set_lists))
        finally:
            got.free()
    finally:
        want.free()
        for dp in pools:
            dp.free()


# ---- 5. fills

@pytest.mark.parametrize("k,seed,n", [(31, 42, 94), (63, 74, 62), (95, 106, 62)])
def test_fills_on_the_device_pool_graph_equal_fills_on_the_pool_graph(P, k, seed, n):
    seqs, set_lists, shared, set_shared, gaps, gap_set = PC.fill_workload(k, seed, n)
    assert gap_set == list(range(len(set_lists)))
    reach = [(_gap(P, g), P.reach_radius(_gap(P, g), PC.D_ERR)) for g in gaps]   # (the sound radius: no fill changes)
    cut = len(seqs) // 2 + 1
    pools = [_held(P, DC.pool_bam(seqs[:cut])), _held(P, DC.pool_bam(seqs[cut:]))]
    try:
        u, hook = _device_build(P, pools, set_lists, k, 1, shared=shared, set_shared=set_shared, reach=reach)
        for dp in pools:   # (a build keeps no pointer into a pool)
            dp.free()
        w = P.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared, reach=reach)
        try:
            assert hook["text_bytes_packed_on_host"] == 0
            assert hook["text_bytes_gathered_on_device"] == _in_use_positions(seqs, set_lists, shared, set_shared)
            assert u.validate() == (0, "")
            got = _fill(P, u, gaps, gap_set)
            want = _fill(P, w, gaps, gap_set)
        finally:
            u.free()
            w.free()
    finally:
        for dp in pools:
            dp.free()
    for i in range(len(gaps)):
        assert _fields(got[i]) == _fields(want[i]), "gap %d (set %d)" % (i, gap_set[i])
    assert sum(r.count > 0 for r in got) > len(gaps) // 3


# ---- 6. Gap2Seq-libraries

def test_libraries_output_does_not_depend_on_the_device_pool(P, tmp_path):
    assert os.access(EXE, os.X_OK), "Gap2Seq-libraries was not built"
    libs, records, bed = libraries_case()
    for i, (data, _, _, _) in enumerate(libs):
        (tmp_path / ("lib%d.bam" % i)).write_bytes(data)
    (tmp_path / "gaps.fa").write_text("".join(records))
    (tmp_path / "gaps.bed").write_text("".join(bed))
    (tmp_path / "libs.txt").write_text("".join("%s\t%d\t%d\t%g\n" % (tmp_path / ("lib%d.bam" % i), m, s, t)
                                               for i, (_, m, s, t) in enumerate(libs)))
    seen = []
    # (where the pools lay: all three on the device, or all three on the host with the filter there)
    runs = ((["-device-pool", "0"], None), (["-device-pool", "1"], "3 of 3 pools held on the device"),
            (["-device-pool", "1", "-filter-device", "-1"], "0 of 3 pools held on the device"))
    for extra, want in runs:
        out = tmp_path / ("out%d.fa" % len(seen))
        argv = [EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
                str(tmp_path / "gaps.bed"), "-filled", str(out), "-k", str(K), "-fuz", str(FUZ), "-solid", str(SOLID),
                "-dist-error", str(DERR), "-randseed", str(LSEED)] + extra
        env = dict(os.environ, G2S_DEBUG="1")
        run = subprocess.run(argv, capture_output=True, text=True, timeout=300, env=env)
        assert run.returncode == 0, run.stderr
        seen.append((out.read_bytes(), run.stdout.strip().splitlines()[-1]))
        assert ("pools held on the device" in run.stderr) == (want is not None) and (want or "") in run.stderr, run.stderr[-2000:]
    assert seen[0] == seen[1] == seen[2]
    assert int(seen[0][1].split()[1]) >= 12   # (Filled X out of 16 gaps)
