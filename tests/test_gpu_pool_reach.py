"""Pooled set graphs bounded by reach records on the MI355X (gap2seq_amd/csrc/dbg_gpu.hip: k_reach_bfs, the bounded
search per set over the run tables): the device build against the host build and the brute-force model; the hook; the
fills on a bounded graph against the fills on the whole graph and the CPU oracle, gap by gap, at the sound radius; a
radius too small, which must change a fill; Gap2Seq-libraries with and without G2S_NO_REACH; the queue's overflow path."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import cases  # noqa: E402
import oracle_lib as O  # noqa: E402
import pool_cases as PC  # noqa: E402
import reach_cases as RC  # noqa: E402
import test_gpu_read_pool as RP  # noqa: E402  (the libraries case and its restatement; nothing of it is changed)

pytestmark = pytest.mark.gpu

SEED = 7


def _device_reach(product, monkeypatch, capfd, seqs, set_lists, k, solid, shared, set_shared, reach):
    """from_pool with reach records on the device; the G2S_DEBUG line must say so"""
    monkeypatch.delenv("G2S_HOST_BUILD", raising=False)
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    u = product.Graph.from_pool(seqs, set_lists, k, solid, shared=shared, set_shared=set_shared, reach=reach)
    err = capfd.readouterr().err
    monkeypatch.delenv("G2S_DEBUG")
    assert "pooled set graph build" in err and "on the GPU" in err and "reach:" in err, err[-2000:]
    return u


def _host_reach(product, monkeypatch, seqs, set_lists, k, solid, shared, set_shared, reach):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    try:
        return product.Graph.from_pool(seqs, set_lists, k, solid, shared=shared, set_shared=set_shared, reach=reach)
    finally:
        monkeypatch.delenv("G2S_HOST_BUILD")


def _pool_reach(product, seqs, set_lists, k, radius):
    """records for tests/pool_cases.pool_workload: flanks cut from its reads A, B and X; every third set without one"""
    a, b, x = seqs[0], seqs[1], seqs[6]
    gaps = [product.Gap(a[40:40 + k + 3], b[150:150 + k + 2], 60, 3, 2), product.Gap(x[20:20 + k + 1], a[200:200 + k + 4], 30, 1, 4),
            product.Gap(b[10:10 + k], b[300:300 + k], 200, 0, 0)]
    return [None if s % 3 == 2 else (gaps[(s + s // 3) % 3], radius) for s in range(len(set_lists))]


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", [31, 63, 95])
def test_device_reach_build_equals_host_reach_build(product, monkeypatch, capfd, k, solid):
    for mode in ("shared", "empty", "none"):
        seqs, set_lists, shared, set_shared = PC.pool_workload(k, mode)
        for radius in (0, 25, 2000):
            reach = _pool_reach(product, seqs, set_lists, k, radius)
            dev = _device_reach(product, monkeypatch, capfd, seqs, set_lists, k, solid, shared, set_shared, reach)
            info, pool = product.test_last_pool_reach(), product.test_last_pool_build()
            host = _host_reach(product, monkeypatch, seqs, set_lists, k, solid, shared, set_shared, reach)
            hinfo = product.test_last_pool_reach()
            try:
                PC.assert_same_graph(dev, host, len(set_lists))
                assert info["on_device"] == 1 and hinfo["on_device"] == 0 and info["full_kmers"] is None
                assert info["reach_sets"] == hinfo["reach_sets"] == sum(r is not None for r in reach)
                assert info["kept_kmers"] == hinfo["kept_kmers"] and info["levels"] == hinfo["levels"] <= radius
                assert hinfo["kept_kmers"] <= hinfo["full_kmers"]
                assert pool["on_device"] == 1 and pool["keys_sorted"] == pool["own_positions"] + pool["shared_positions"]
            finally:
                dev.free()
                host.free()


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", [31, 63, 95])
def test_device_reach_build_equals_the_model(product, monkeypatch, capfd, k, solid):
    seqs, set_lists, shared, set_shared, gaps = RC.reach_workload(k, solid)
    for radius in (1, 12, 400):
        dev = _device_reach(product, monkeypatch, capfd, seqs, set_lists, k, solid, shared, set_shared,
                            RC.reach_list(product, gaps, radius))
        try:
            radii = [None if s in RC.NO_RECORD else radius for s in range(len(set_lists))]
            sizes = RC.assert_matches_model(dev, seqs, set_lists, shared, set_shared, gaps, radii, k, solid)
            for s in (0, 5, 6):
                assert 0 < sizes[s][1] < sizes[s][0], (s, radius, sizes[s])
        finally:
            dev.free()


def _fill_reach(product, gaps, gap_set, nsets, radius_of):
    reach = [None] * nsets
    for g, s in zip(gaps, gap_set):
        gp = product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"])
        reach[s] = (gp, radius_of(gp))
    return reach


@pytest.mark.parametrize("k", [31, 63, 95])
def test_device_reach_build_on_lists_of_gaps(product, monkeypatch, capfd, k):
    """fill_workload-sized lists with 1, 5 and 40 flagged sets, every set with a record"""
    for nflag in (1, 5, 40):
        seqs, set_lists, shared, set_shared, gaps, gap_set = PC.fill_workload(k, 19, 46, flag=lambda s, n=nflag: s < n)
        reach = _fill_reach(product, gaps[:-2], gap_set[:-2], len(set_lists), lambda gp: product.reach_radius(gp, PC.D_ERR))
        reach[-1] = reach[0]
        dev = _device_reach(product, monkeypatch, capfd, seqs, set_lists, k, 1, shared, set_shared, reach)
        info, pool = product.test_last_pool_reach(), product.test_last_pool_build()
        whole = product.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared)
        host = _host_reach(product, monkeypatch, seqs, set_lists, k, 1, shared, set_shared, reach)
        try:
            PC.assert_same_graph(dev, host, len(set_lists))
            own = sum(len(seqs[i]) + 1 for lst in set_lists for i in lst)
            sh = sum(len(seqs[i]) + 1 for i in shared)
            assert pool == dict(own_positions=own, shared_positions=sh, keys_sorted=own + sh, on_device=1)
            assert info["on_device"] == 1 and info["reach_sets"] == len(set_lists) - 1
            assert 0 < dev.num_kmers < whole.num_kmers
            assert dev.set_nodes(len(set_lists) - 2)[1] == whole.set_nodes(len(set_lists) - 2)[1]  # (no record: the whole set)
        finally:
            dev.free()
            whole.free()
            host.free()


@pytest.mark.parametrize("k", [31, 63, 95])
def test_one_set_with_a_record_on_the_device(product, monkeypatch, capfd, k):
    """nsets == 1 with a record (a chunk of Gap2Seq-libraries that holds one gap): built on the device as two sets, the
    second empty, and handed back as an ordinary graph — the model's k-mers, the host build's graph, and a fill"""
    seqs, set_lists, shared, set_shared, gaps = RC.reach_workload(k, 1)
    g = gaps[0]
    reach = [(product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"]), 40)]
    dev = _device_reach(product, monkeypatch, capfd, seqs, [set_lists[0]], k, 1, shared, [1], reach)
    info = product.test_last_pool_reach()
    host = _host_reach(product, monkeypatch, seqs, [set_lists[0]], k, 1, shared, [1], reach)
    try:
        full, kept, _ = RC.model_set(seqs, set_lists[0], shared, True, g, 40, k, 1)
        assert info["on_device"] == 1 and info["reach_sets"] == 1 and info["kept_kmers"] == len(kept)
        assert dev.num_sets == host.num_sets == 1 and dev.num_kmers == host.num_kmers == len(kept) and 0 < len(kept) < len(full)
        assert dev.num_unitigs == host.num_unitigs and dev.set_nodes(0) == (0, len(kept))
        for x in full:
            v = dev.node(x)
            assert (v != product.G2S_INVALID_NODE) == (x in kept) and (host.node(x) != product.G2S_INVALID_NODE) == (x in kept)
            if x in kept:
                assert sorted(dev.node_string(w) for w in dev.successors(v)) == RC.successors(dev.node_string(v), kept)
                assert sorted(dev.node_string(w) for w in dev.successors(v ^ 1)) == RC.successors(dev.node_string(v ^ 1), kept)
        assert dev.validate() == (0, "") and host.validate() == (0, "")
        got = _fill(product, dev, [g], [0], 100)[0]
        want = _fill(product, host, [g], [0], 100)[0]
        assert RP._fields(got) == RP._fields(want)
    finally:
        dev.free()
        host.free()


def test_a_queue_that_overflows_grows_and_the_search_runs_again(product, monkeypatch, capfd):
    """a flagged set without own reads whose seeds lie in a long shared read: it keeps more k-mers than the queue's
    first size (the own runs + 4 096 a set with a record), so the queue is made larger and the searches run again — on
    the device, with the host build's graph"""
    k = 31
    rng = cases.SplitMix(4242)
    genome = cases.random_dna(rng, 12000)
    seqs = [genome, cases.random_dna(rng, 400)]
    g = product.Gap(genome[6000 - k - 2:6000], genome[6100:6100 + k + 2], 100 + k, 2, 2)
    reach = [(g, 100000), None]
    monkeypatch.delenv("G2S_HOST_BUILD", raising=False)
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    dev = product.Graph.from_pool(seqs, [[], [1]], k, 1, shared=[0], set_shared=[1, 0], reach=reach)
    err = capfd.readouterr().err
    monkeypatch.delenv("G2S_DEBUG")
    info = product.test_last_pool_reach()
    host = _host_reach(product, monkeypatch, seqs, [[], [1]], k, 1, [0], [1, 0], reach)
    try:
        assert "reach: the queue of 4096 k-mers overflowed, searching again with 11970" in err, err[-2000:]
        assert "on the GPU" in err and info["on_device"] == 1 and info["kept_kmers"] == 12000 - k + 1 > 4096
        PC.assert_same_graph(dev, host, 2)
    finally:
        dev.free()
        host.free()


# ---- fills on a bounded graph

def _fill(product, graph, gaps, gap_set, d_err):
    sess = product.Session(graph, 0, d_err=d_err, randseed=SEED)
    try:
        return sess.fill_sets([product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"]) for g in gaps], gap_set)
    finally:
        sess.destroy()


def _oracle_sequence(seqs, g, k, d_err):
    if not seqs:
        return g["left"] + "N" * g["gap_len"] + g["right"]
    og = O.OracleGraph(seqs, k, 1)
    try:
        fa, _ = O.execute_single(og, g["left"], g["right"], g["gap_len"], k, solid=1, d_err=d_err,
                                 max_fuz=max(g["lmf"], g["rmf"], PC.FUZ), randseed=SEED)
    finally:
        og.free()
    return "".join(ln for ln in fa.splitlines() if not ln.startswith(">"))


@pytest.mark.parametrize("resident", ["0", "1"])
@pytest.mark.parametrize("k,seed,n,d_err", [(31, 42, 94, 500), (63, 74, 62, 500), (95, 106, 62, 500), (31, 43, 40, 2000)])
def test_fills_on_the_reach_graph_equal_fills_on_the_whole_graph(product, monkeypatch, capfd, k, seed, n, d_err, resident):
    """the point of the feature: at the sound radius nothing of any fill is lost — record fields and fill text equal
    the whole graph's, and the sequence equals the CPU oracle's on the gap's expanded reads.  d_err 2000: the radius
    exceeds the diameter of every set (the deep case)."""
    monkeypatch.setenv("G2S_RESIDENT", resident)
    seqs, set_lists, shared, set_shared, gaps, gap_set = PC.fill_workload(k, seed, n)
    sets = PC.expanded(seqs, set_lists, shared, set_shared)
    reach = _fill_reach(product, gaps[:-2], gap_set[:-2], len(set_lists), lambda gp: product.reach_radius(gp, d_err))
    reach[-2], reach[-1] = reach[0], reach[0]   # (the two sets without own reads are named by copies of the first gap)
    u = _device_reach(product, monkeypatch, capfd, seqs, set_lists, k, 1, shared, set_shared, reach)
    w = product.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared)
    try:
        assert 0 < u.num_kmers < w.num_kmers
        got = _fill(product, u, gaps, gap_set, d_err)
        want = _fill(product, w, gaps, gap_set, d_err)
    finally:
        u.free()
        w.free()
    filled = flagged_filled = 0
    for i, g in enumerate(gaps):
        assert RP._fields(got[i]) == RP._fields(want[i]), "gap %d (set %d)" % (i, gap_set[i])
        assert RP._sequence(g, got[i]) == _oracle_sequence(sets[gap_set[i]], g, k, d_err), "gap %d (set %d)" % (i, gap_set[i])
        filled += got[i].count > 0
        flagged_filled += got[i].count > 0 and set_shared[gap_set[i]] == 1
    assert filled > len(gaps) // 3 and flagged_filled > sum(set_shared) // 3


def test_a_radius_too_small_changes_the_fill(product, monkeypatch, capfd):
    """One read, one path: the last k-mer of the left flank and the first of the right flank are L = true_len + k steps
    apart, and the claimed length is the smallest the fill accepts for that path (gap_len + d_err = L: the oracle,
    asked first, fills the gap and does not fill it at gap_len - 1), so the only closing path has the maximal length
    and the sound radius is L + lmf + rmf.
    The kept set is the union of the balls around ALL seeds, the right flank's k-mers included, so a closing path of
    L steps loses a k-mer only once 2 * radius < L - 1.  Hence the fill at sound - 1 is still the whole graph's — the
    definition keeps more than the search's depth bound needs whenever the path closes; measured here: equal at
    radius 141 (sound), 140 and 65 — and the first radius that must change it is (L - 1) // 2 - 1 = 64: the middle of
    the path is gone and the gap is no longer filled.  That is where the pruning bites, and the test pins both sides."""
    k, d_err, true_len, fuz = 31, 50, 100, 5
    rng = cases.SplitMix(77)
    read = cases.random_dna(rng, 500)
    L = true_len + k
    g = dict(left=read[150 - k - fuz:150], right=read[150 + true_len:150 + true_len + k + fuz], gap_len=L - d_err, lmf=fuz, rmf=fuz)
    assert "N" not in _oracle_sequence([read], g, k, d_err)                      # filled at the maximal length ...
    assert "N" in _oracle_sequence([read], dict(g, gap_len=g["gap_len"] - 1), k, d_err)   # ... and not beyond it
    gp = product.Gap(g["left"], g["right"], g["gap_len"], fuz, fuz)
    sound = product.reach_radius(gp, d_err)
    assert sound == L + 2 * fuz
    seqs, set_lists = [read, cases.random_dna(rng, 300)], [[0], [1]]
    whole = product.Graph.from_pool(seqs, set_lists, k, 1)
    want = _fill(product, whole, [g], [0], d_err)[0]
    n_whole = whole.set_nodes(0)[1]
    whole.free()
    assert want.count > 0 and RP._sequence(g, want) == _oracle_sequence([read], g, k, d_err)
    half = (L - 1) // 2
    seen = {}
    for radius in (sound, sound - 1, half, half - 1):
        u = _device_reach(product, monkeypatch, capfd, seqs, set_lists, k, 1, None, None, [(gp, radius), None])
        try:
            seen[radius] = (u.set_nodes(0)[1], _fill(product, u, [g], [0], d_err)[0])
        finally:
            u.free()
        print("radius %d: %d of %d k-mers, count %d" % (radius, seen[radius][0], n_whole, seen[radius][1].count))
    for radius in (sound, sound - 1, half):
        assert RP._fields(seen[radius][1]) == RP._fields(want), radius
    assert seen[sound - 1][0] < seen[sound][0] < n_whole                         # (the read goes on beyond both balls)
    cut = seen[half - 1]
    assert cut[0] < seen[half][0]                                                 # (the two k-mers in the middle of the path among them)
    assert RP._fields(cut[1]) != RP._fields(want) and cut[1].count <= 0


# ---- Gap2Seq-libraries

def test_libraries_output_is_the_same_with_and_without_reach(product, tmp_path):
    assert os.access(RP.EXE, os.X_OK), "Gap2Seq-libraries was not built"
    libs, records, bed = RP.libraries_case()
    for i, (data, _, _, _) in enumerate(libs):
        (tmp_path / ("lib%d.bam" % i)).write_bytes(data)
    (tmp_path / "gaps.fa").write_text("".join(records))
    (tmp_path / "gaps.bed").write_text("".join(bed))
    (tmp_path / "libs.txt").write_text("".join("%s\t%d\t%d\t%g\n" % (tmp_path / ("lib%d.bam" % i), m, s, t)
                                               for i, (_, m, s, t) in enumerate(libs)))
    _, _, took, _ = RP.restatement(libs, [r.rstrip("\n") for r in records], bed, fill=False)
    assert any(took) and not all(took)
    outs, logs = [], []
    for no_reach in (None, "1"):
        env = dict(os.environ, G2S_DEBUG="1")
        env.pop("G2S_NO_REACH", None)
        if no_reach:
            env["G2S_NO_REACH"] = no_reach
        out = tmp_path / ("out%s.fa" % (no_reach or "0"))
        run = subprocess.run([RP.EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
                              str(tmp_path / "gaps.bed"), "-filled", str(out), "-k", str(RP.K), "-fuz", str(RP.FUZ), "-solid",
                              str(RP.SOLID), "-dist-error", str(RP.DERR), "-randseed", str(RP.LSEED)], capture_output=True,
                             text=True, timeout=300, env=env)
        assert run.returncode == 0, run.stderr
        outs.append(out.read_bytes())
        logs.append(run.stderr)
    assert outs[0] == outs[1] and outs[0].count(b">") == len(records)
    assert "reach:" in logs[0] and "reach:" not in logs[1]


# ---- the queue's overflow path

def test_a_queue_too_small_lands_on_the_host_build(product, monkeypatch, capfd):
    k = 31
    seqs, set_lists, shared, set_shared, gaps = RC.reach_workload(k, 1)
    reach = RC.reach_list(product, gaps, 400)
    want = _host_reach(product, monkeypatch, seqs, set_lists, k, 1, shared, set_shared, reach)
    monkeypatch.setenv("G2S_REACH_QUEUE_CAP", "64")
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    got = product.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared, reach=reach)
    err = capfd.readouterr().err
    info = product.test_last_pool_reach()
    try:
        assert "pooled set graph on the host (reach: the search's queue of 64 k-mers" in err, err[-2000:]
        assert info["on_device"] == 0 and info["full_kmers"] is None  # (behind a device build that gave up: not counted)
        PC.assert_same_graph(got, want, len(set_lists))
    finally:
        got.free()
        want.free()
