"""Graph builds at even k on the MI355X (gap2seq_amd/csrc/dbg_gpu.hip): rank-space tables with the palindrome rules and
the predecessor table, unitig numbering by list ranking, id-space tables — single graphs, set graphs, pooled set graphs
and pooled set graphs with reach records, each against the host build (G2S_HOST_BUILD=1, the authority:
tests/test_even_k_host.py) and pyref.Graph / the brute-force reach model; fills on a device-built graph against fills
on the host-built graph and the CPU oracle; and odd k, which must not gain a predecessor table."""
import pytest

import cases
import even_k_cases as EK
import pool_cases as PC
import pyref
import reach_cases as RC
from test_gpu_parity import _check_batch, _gaps, _result_tuple

pytestmark = pytest.mark.gpu

SEED = 7
ON_GPU = "tables, unitig order, id space:"


def _both(product, monkeypatch, capfd, build):
    """(device-built graph, host-built graph, the device build's G2S_DEBUG text)"""
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    host = build()
    monkeypatch.delenv("G2S_HOST_BUILD")
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    dev = build()
    err = capfd.readouterr().err
    monkeypatch.delenv("G2S_DEBUG")
    return dev, host, err


# ---- single graphs

@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", [2, 4, 12, 30, 32, 64, 96, 126])
def test_single_graph_build_at_even_k(product, monkeypatch, capfd, tmp_path, k, solid):
    reads, designed = EK.designed_reads(k, solid)
    dev, host, err = _both(product, monkeypatch, capfd, lambda: product.Graph.from_seqs(reads, k, solid))
    try:
        line = [ln for ln in err.splitlines() if ON_GPU in ln]
        assert len(line) == 1 and line[0].endswith("on the GPU") and "GPU sort" in err, err[-2000:]
        assert dev.num_kmers == host.num_kmers > 0 and dev.num_unitigs == host.num_unitigs
        mh = EK.assert_graph_is_pyrefs(host, reads, k, solid, designed)  # (the designed palindromes are there)
        md = EK.assert_graph_is_pyrefs(dev, reads, k, solid, designed)
        assert md == mh
        # the graph's device copy holds the predecessor table, as an uploaded host-built graph's does
        host.upload(0)
        assert dev.device_bytes(0) == host.device_bytes(0) > 2 * 32 * dev.num_kmers
        if k in (30, 64):
            path = str(tmp_path / "g.bin")
            dev.save(path)
            back = product.Graph.load(path)
            try:
                assert EK.graph_map(back) == md and back.num_unitigs == dev.num_unitigs and back.validate() == (0, "")
            finally:
                back.free()
    finally:
        dev.free()
        host.free()


def test_odd_k_build_keeps_no_predecessor_table(product, monkeypatch, capfd):
    k = 31
    reads, _ = EK.designed_reads(30, 1)
    dev, host, err = _both(product, monkeypatch, capfd, lambda: product.Graph.from_seqs(reads, k, 1))
    try:
        assert any(ON_GPU in ln and ln.endswith("on the GPU") for ln in err.splitlines()), err[-2000:]
        n = dev.num_kmers
        words = (n + 63) // 64 + 1
        # the successor table and the padded unitig-start bitmap, nothing else
        assert dev.device_bytes(0) == 32 * n + 8 * (words + 2 * 64)
        host.upload(0)
        assert host.device_bytes(0) == dev.device_bytes(0)
        m = EK.graph_map(dev)
        assert m == EK.graph_map(host)
        for s, (_, pred) in m.items():  # predecessors still come from the successor table
            assert list(pred) == [y for y in (nt + s[:-1] for nt in "TGAC") if y in m], s
    finally:
        dev.free()
        host.free()


# ---- set graphs

def _set_workload(k, seed, ngaps, solid):
    """the workload shape of tests/test_gpu_sets.py (_workload): per gap, reads of both haplotypes around the gap plus
    a window from elsewhere; every fourth gap shares the set in front of it; a set named by no gap; an empty set"""
    hap = cases.toy_genome(seed, 12000, k, repeats=6, tandem=2, snp_every=350)
    genome = hap[0]
    rng = cases.SplitMix(seed * 31 + k)
    raw = cases.cut_gaps(seed, genome, k, 10, ngaps, 10, 160, 100)
    sets = []
    for i, g in enumerate(raw):
        pos = genome.find(g["left"]) + len(g["left"])
        lo, hi = max(0, pos - 150), min(len(genome), pos + g["true_len"] + 150)
        o = rng.randint(0, len(genome) - 400)
        reads = ([h[lo:hi] for h in hap] + [genome[o:o + 400]]) * solid
        if i % 4 == 3:
            sets[-1].extend(reads)
        else:
            sets.append(reads)
    sets.append([genome[:600]] * solid)
    sets.append([])
    return sets


def _hairpin(rng, k):
    """(read, the palindrome at its centre, the k-mer in front of it)"""
    s = cases.random_dna(rng, k + 25)
    read, at = s + pyref.revcomp(s), len(s) - k // 2
    assert read[at:at + k] == pyref.revcomp(read[at:at + k])
    return read, read[at:at + k], read[at - 1:at - 1 + k]


@pytest.mark.parametrize("k", [30, 62, 94])
def test_set_build_at_even_k(product, monkeypatch, capfd, k):
    sets = _set_workload(k, 101 + k, 40, solid=2)
    rng = cases.SplitMix(k)
    unit = cases.random_dna(rng, k + 19)
    sets.insert(3, [unit * 4] * 2)               # one circular unitig
    sets.insert(7, [unit * 4, cases.random_dna(rng, 300)] * 2)
    sets.insert(9, [cases.random_dna(rng, 200)])  # every k-mer once: nothing solid at 2
    hairpin, pal, before = _hairpin(rng, k)
    with_hairpin = (0, 3, 5, 7, 12)
    for s in with_hairpin:
        sets[s] += [hairpin] * 2
    dev, host, err = _both(product, monkeypatch, capfd, lambda: product.Graph.from_sets(sets, k, 2))
    try:
        assert "set graph build" in err and "on the GPU" in err and "on the host" not in err, err[-2000:]
        PC.assert_same_graph(dev, host, len(sets))
        assert host.validate() == (0, "") and dev.set_nodes(9)[1] == 0
        for s in with_hairpin:
            for u in (dev, host):
                v = u.set_node(s, pal)
                assert v != product.G2S_INVALID_NODE and u.node_string(v) == pal
                assert len(u.successors(v)) == 1 and u.successors(v ^ 1) == [] and u.predecessors(v ^ 1) == []
                assert [u.node_string(w) for w in u.predecessors(v)] == [before]
        assert dev.set_node(1, pal) == product.G2S_INVALID_NODE
        host.upload(0)
        assert dev.device_bytes(0) == host.device_bytes(0)
    finally:
        dev.free()
        host.free()


# ---- pooled set graphs, without and with reach records

K_POOL = 30


def _pool_with_hairpin(mode):
    """tests/pool_cases.py: pool_workload at k = 30 with a hairpin read in several own lists and in the shared list"""
    seqs, set_lists, shared, set_shared = PC.pool_workload(K_POOL, mode)
    hairpin, pal, _ = _hairpin(cases.SplitMix(30), K_POOL)
    seqs = seqs + [hairpin]
    h = len(seqs) - 1
    set_lists = [list(lst) for lst in set_lists]
    for s in (0, 2, 5):
        set_lists[s] += [h, h]
    if mode == "shared":
        shared = shared + [h, h]
    return seqs, set_lists, shared, set_shared, pal


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("mode", ["shared", "empty", "none"])
def test_pool_build_at_even_k(product, monkeypatch, capfd, mode, solid):
    seqs, set_lists, shared, set_shared, pal = _pool_with_hairpin(mode)
    infos = []

    def build():
        g = product.Graph.from_pool(seqs, set_lists, K_POOL, solid, shared=shared, set_shared=set_shared)
        infos.append(product.test_last_pool_build())
        return g
    dev, host, err = _both(product, monkeypatch, capfd, build)
    try:
        assert "pooled set graph build" in err and "on the GPU" in err, err[-2000:]
        hinfo, info = infos
        assert info["on_device"] == 1 and hinfo["on_device"] == 0
        assert info["keys_sorted"] == info["own_positions"] + info["shared_positions"]
        PC.assert_same_graph(dev, host, len(set_lists))
        for s in (0, 2, 5) + ((1, 3) if mode == "shared" else ()):
            assert dev.set_node(s, pal) != product.G2S_INVALID_NODE and host.set_node(s, pal) != product.G2S_INVALID_NODE
        assert dev.set_node(4, pal) == product.G2S_INVALID_NODE
    finally:
        dev.free()
        host.free()


def _assert_kept_is_the_models(u, seqs, set_lists, shared, set_shared, gaps, radii, k, solid):
    """every set's k-mers against the brute-force model of tests/reach_cases.py; [(full, kept)] sizes"""
    sizes = []
    for s, own in enumerate(set_lists):
        full, kept, _ = RC.model_set(seqs, own, shared, bool(set_shared[s]), gaps[s], radii[s], k, solid)
        assert u.set_nodes(s)[1] == len(kept), "set %d: %d k-mers, the model keeps %d of %d" % (s, u.set_nodes(s)[1], len(kept), len(full))
        for x in full:
            v = u.set_node(s, x)
            assert (v != RC_INVALID) == (x in kept), "set %d k-mer %s" % (s, x)
            if x in kept:
                assert sorted(u.node_string(w) for w in u.successors(v)) == RC.successors(u.node_string(v), kept), (s, x)
        sizes.append((len(full), len(kept)))
    return sizes


RC_INVALID = 0xFFFFFFFF


def _reach_workload_with_a_palindromic_seed(solid):
    """tests/reach_cases.py: reach_workload at k = 30, plus a flagged set 8 whose gap's left flank IS a palindromic
    k-mer (lmf = 0: the one left seed), inside a window that the shared list extends"""
    k = K_POOL
    seqs, set_lists, shared, set_shared, gaps = RC.reach_workload(k, solid)
    rng = cases.SplitMix(3030)
    a, b, tail = cases.random_dna(rng, 70), cases.random_dna(rng, 150), cases.random_dna(rng, 200)
    pal = EK.palindrome(rng, k)
    seqs = seqs + [a + pal + b, b[-(k + 5):] + tail]
    own, ext = len(seqs) - 2, len(seqs) - 1
    set_lists = set_lists + [[own] * solid]
    set_shared = set_shared + [1]
    shared = shared + [ext] * solid
    gaps = gaps + [dict(left=pal, right=b[40:40 + k + 2], gap_len=40 + k, lmf=0, rmf=2)]
    return seqs, set_lists, shared, set_shared, gaps, pal


@pytest.mark.parametrize("solid", [1, 2])
def test_pool_reach_build_at_even_k(product, monkeypatch, capfd, solid):
    k = K_POOL
    seqs, set_lists, shared, set_shared, gaps, pal = _reach_workload_with_a_palindromic_seed(solid)
    assert RC.seeds_of(gaps[8], k)[0] == pal
    for radius in (0, 1, 12, 400):
        reach = RC.reach_list(product, gaps, radius)
        infos = []

        def build():
            g = product.Graph.from_pool(seqs, set_lists, k, solid, shared=shared, set_shared=set_shared, reach=reach)
            infos.append((product.test_last_pool_reach(), product.test_last_pool_build()))
            return g
        dev, host, err = _both(product, monkeypatch, capfd, build)
        try:
            assert "pooled set graph build" in err and "on the GPU" in err and "reach:" in err, err[-2000:]
            (hinfo, _), (info, pool) = infos
            assert info["on_device"] == 1 and hinfo["on_device"] == 0 and pool["on_device"] == 1
            assert pool["keys_sorted"] == pool["own_positions"] + pool["shared_positions"]
            assert info["kept_kmers"] == hinfo["kept_kmers"] and info["levels"] == hinfo["levels"] <= radius
            PC.assert_same_graph(dev, host, len(set_lists))
            radii = [None if s in RC.NO_RECORD else radius for s in range(len(set_lists))]
            sizes = _assert_kept_is_the_models(dev, seqs, set_lists, shared, set_shared, gaps, radii, k, solid)
            # the palindromic seed is claimed once and is a node of its set, on strand 1 only
            v = dev.set_node(8, pal)
            assert v != product.G2S_INVALID_NODE and dev.successors(v ^ 1) == []
            assert 0 < sizes[8][1] and (radius >= 400 or sizes[8][1] < sizes[8][0]), (radius, sizes[8])
            if radius == 0:
                assert sizes[8][1] == len({x for x in RC.seeds_of(gaps[8], k)})
        finally:
            dev.free()
            host.free()


# ---- fills

def _fields(r):
    return (r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, r.substats, r.phaseC_count, r.lengths)


def _fill_fixture(k):
    """a 30 kbp toy genome (repeats, tandem arrays, a second haplotype) with 40 gaps and the hairpins and inversions
    of cases.strand_flip_genome with their gaps: about 50 gaps"""
    seqs = cases.toy_genome(k + 300, 30000, k, repeats=8, tandem=3, snp_every=500)
    e = k + 20
    gaps = cases.cut_gaps(k + 300, seqs[0], k, 10, 40, 20, 300, e)
    fseqs, fgaps = cases.strand_flip_genome(k, 4000, k)
    return seqs + fseqs, gaps + fgaps[:10], e


def test_fills_on_the_device_built_graph_at_k32(product, oracle, monkeypatch, capfd):
    k = 32
    seqs, gaps, e = _fill_fixture(k)
    assert 45 <= len(gaps) <= 55
    dev, host, err = _both(product, monkeypatch, capfd, lambda: product.Graph.from_seqs(seqs, k, 1))
    try:
        assert any(ON_GPU in ln and ln.endswith("on the GPU") for ln in err.splitlines()), err[-2000:]
        got = []
        for g in (dev, host):
            sess = product.Session(g, 0, d_err=e, randseed=5)
            try:
                got.append([_result_tuple(r) for r in sess.fill_batch(_gaps(product, gaps))])
            finally:
                sess.destroy()
        assert got[0] == got[1]
        assert sum(1 for r in got[0] if r[0] > 0) > len(gaps) // 2
    finally:
        dev.free()
        host.free()
    # the same list on a device-built graph (the default build) against the oracle, gap by gap
    compared, filled, _, _, _ = _check_batch(product, oracle, seqs, k, gaps, e)
    # (the ten strand-flip gaps are Q7 cases by design, outside the bit-exact comparison; two more for chance ones)
    assert compared >= len(gaps) - 12 and filled >= 25, (compared, filled)


def test_fill_sets_on_the_device_built_reach_graph_at_k30(product, monkeypatch, capfd):
    k = K_POOL
    seqs, set_lists, shared, set_shared, gaps, gap_set = PC.fill_workload(k, 42, 46)
    reach = [None] * len(set_lists)
    for g, s in zip(gaps[:-2], gap_set[:-2]):
        gp = product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"])
        reach[s] = (gp, product.reach_radius(gp, PC.D_ERR))
    reach[-2], reach[-1] = reach[0], reach[0]
    dev, host, err = _both(product, monkeypatch, capfd,
                           lambda: product.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared, reach=reach))
    try:
        assert "pooled set graph build" in err and "on the GPU" in err and "reach:" in err, err[-2000:]
        res = []
        for u in (dev, host):
            sess = product.Session(u, 0, d_err=PC.D_ERR, randseed=SEED)
            try:
                res.append(sess.fill_sets(_gaps(product, gaps), gap_set))
            finally:
                sess.destroy()
        for i in range(len(gaps)):
            assert _fields(res[0][i]) == _fields(res[1][i]), "gap %d (set %d)" % (i, gap_set[i])
        assert sum(1 for r in res[0] if r.count > 0) > len(gaps) // 3
    finally:
        dev.free()
        host.free()
